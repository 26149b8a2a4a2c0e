// backtest_replay.h - interface between the host layer (tangency_replay.cpp) and the backtest replay kernel
// (backtest_replay.hip): the daily P&L, weight drift, turnover and weight metrics of many portfolios, one wavefront each.
#pragma once
#include <hip/hip_runtime.h>

#define TP_REPLAY_WAVES 4            // portfolios per 256-thread workgroup
#define TP_REPLAY_METRICS 5          // max_long, max_short, avg_long, avg_short, distance to the value-weighted portfolio
#define TP_REPLAY_KSTATUS_SUM_CHECK 1

// One portfolio (device and host layout).  Offsets and strides are in elements of their flat buffers: weights (double),
// cols (int) and caps (double) share u_off / u_stride; the merge maps prev / next are dense [R x k] at m_off.
struct tp_replay_port_t {
    long long w_off, w_stride;
    long long u_off, u_stride;
    long long m_off;
    double scaling, cost;
    int k, pad;
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
};

// slots of the held universe per lane a portfolio of k assets is instantiated for: 1, 2, 4, 8, 16 or 32 (k <= 2048)
int tp_replay_slots_per_lane(int k);
// launches the portfolios order[first .. first + count), which all have tp_replay_slots_per_lane(k) == spl
hipError_t tp_replay_launch(const tp_replay_args_t& a, int spl, hipStream_t st);
