// backtest_replay.h - interface between the host layer (tangency_replay.cpp) and the backtest replay kernel
// (backtest_replay.hip): the daily P&L, weight drift, turnover and weight metrics of many portfolios, one wavefront each.
#pragma once
#include <hip/hip_runtime.h>

#define TP_REPLAY_WAVES 4            // portfolios per 256-thread workgroup
#define TP_REPLAY_METRICS 5          // max_long, max_short, avg_long, avg_short, distance to the value-weighted portfolio
#define TP_REPLAY_KSTATUS_SUM_CHECK 1
#define TP_REPLAY_KSTATUS_BAD_WEIGHTS 2   // device-fed form: a row was read whose source status was not 0

// One portfolio (device and host layout).  Offsets and strides are in elements of their flat buffers: weights (double),
// cols (int) and caps (double) share u_off / u_stride; the merge maps prev / next are dense [R x k] at m_off.  The device-fed
// form (tp_replay_run_batch) also reads: the status of rebalancing date j at src_status[s_off + j * s_stride], the factor
// w_scale on a source row, and the portfolio's patches [patch_first, patch_end) of patch_date / patch_rows.
struct tp_replay_port_t {
    long long w_off, w_stride;
    long long u_off, u_stride;
    long long m_off;
    double scaling, cost;
    int k, pad;
    long long s_off, s_stride;
    double w_scale;
    int patch_first, patch_end;
};

struct tp_replay_args_t {
    const double* S;                 // [D x ld] simple returns
    const double* rf;                // [D] daily risk-free rate
    const int* reb_day;              // [R] trading-day index of every rebalancing date; reb_day[0] == 0
    const tp_replay_port_t* port;    // [P]
    const int* order;                // portfolios of this launch: order[first .. first + count)
    const double* weights;
    const int* cols;
    const double* caps;
    const int* prev_slot;
    const int* next_slot;
    double* ret;                     // [P x D]
    double* turnover;                // [P x R]
    double* metrics;                 // [P x R x 5]
    int* status;                     // [P]
    int* bad_day;                    // [P]
    int D, R, ld;
    int first, count;
    // device-fed form (src_status != NULL selects it): `weights` is the producing batch's own buffer
    const int* src_status;           // the source's statuses, next to its weights
    const int* patch_date;           // [n_patch] rebalancing date of every patch, sorted by (portfolio, date)
    const double* patch_rows;        // [n_patch x patch_ld] the rows that replace the source's, taken as they are
    int patch_ld;
};

// slots of the held universe per lane a portfolio of k assets is instantiated for: 1, 2, 4, 8, 16 or 32 (k <= 2048)
int tp_replay_slots_per_lane(int k);
// launches the portfolios order[first .. first + count), which all have tp_replay_slots_per_lane(k) == spl; the device-fed form
// of the kernel when a.src_status is set
hipError_t tp_replay_launch(const tp_replay_args_t& a, int spl, hipStream_t st);
