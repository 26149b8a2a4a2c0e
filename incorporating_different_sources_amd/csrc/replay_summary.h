// replay_summary.h - interface between the host layer (tangency_replay.cpp) and the replay summary kernel
// (replay_summary.hip): the statistics of a replay's daily returns at many trading costs, one wavefront per (portfolio, cost).
#pragma once
#include <hip/hip_runtime.h>

#define TP_SUMMARY_WAVES 4           // costs of ONE portfolio per 256-thread workgroup
#define TP_SUMMARY_NSTATS 32         // doubles per record (TP_SUMMARY_STATS of the C-ABI)
#define TP_SUMMARY_KSTATUS_NO_REPLAY 1
#define TP_SUMMARY_KSTATUS_NONFINITE 2

struct tp_summary_args_t {
    const double* ret;               // [P x D] the replay's daily returns (day 0 is not read)
    const double* turnover;          // [P x R] (date 0 is not read)
    const int* rstatus;              // [P] the replay's statuses
    const int* reb_day;              // [R]
    const int* day_date;             // [D] the rebalancing date j >= 1 that falls on trading day d, or -1
    const double* cost_bp;           // [C]
    const double* rf_excess;         // [D]
    double* stats;                   // [P x C x TP_SUMMARY_NSTATS]
    int* status;                     // [P x C]
    int P, D, R, C;
};

hipError_t tp_summary_launch(const tp_summary_args_t& a, hipStream_t st);
