// backtest_replay.hip - the daily loop of a backtest (ref:1127-1219: mark to market, weight drift, rebalance, turnover
// ref:1054-1075, weight metrics, distance to the value-weighted portfolio ref:1077-1104) for MANY portfolios whose weights are
// already in hand: ONE WAVEFRONT PER PORTFOLIO, four portfolios per 256-thread workgroup.
//
// The loop is sequential in days, independent across portfolios and parallel across assets.  Lane l owns slots l, l+64, ... of
// the held universe; the held weights stay in registers (SPL slots per lane: 1, 2, 4, 8, 16 or 32).  The waves of a workgroup
// share nothing: no barrier, no spin, every loop is bounded by D, R or k.  A wave's own LDS slice holds the drifted weights of
// a rebalancing day for the one cross-lane access of the loop, the turnover's gather through the merge map.
//
// Every sum is a lane-local partial sum in slot order followed by a fixed 64-lane tree (DPP rotations inside the rows of 16, v_readlane across them): bit-reproducible from run to run
// and independent of the other portfolios of the launch.  Compiled with -ffp-contract=off: the operations are the host's
// (`_replay_backtest`), one rounding each.
//
// Loads.  The returns of day d+1 (and rf[d+1]) do not depend on the weights: they are requested at the top of day d, ahead of
// its reductions (the universe of the NEXT rebalancing date is kept in registers one rebalance ahead, so this also holds on a
// rebalancing day); up to 8 slots per lane the rebalancing inputs are requested there too.
//
// Two forms, chosen at compile time.  FED = false: the weights are the caller's, uploaded (tp_replay_run).  FED = true: they
// lie where a batch's run or sweep wrote them (tp_replay_run_batch): a row is scaled by the portfolio's w_scale and carries the
// status of its source entry, or it is replaced by a patch row.  The patches of a portfolio are sorted by date and the dates of
// the loop rise, so the wave keeps a cursor into them and the next patched date as wave-uniform scalars and compares once per
// rebalancing date: no search, and the row pointer, the scale and the status are selected, not branched on - the control flow
// around the reductions stays wave-uniform.
#include "backtest_replay.h"
#include "replay_wave_prims.h"

namespace {

template <int SPL, bool FED>
__global__ __launch_bounds__(64 * TP_REPLAY_WAVES) void replay_kernel(const tp_replay_args_t a) {
    __shared__ double lds_all[TP_REPLAY_WAVES][SPL * 64];
    constexpr bool EARLY = SPL <= 8;          // rebalancing inputs requested ahead of the day's reductions
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int idx = blockIdx.x * TP_REPLAY_WAVES + wave;
    if (idx >= a.count) return;               // (a whole wave; the waves of a workgroup never meet)
    const int p = a.order[a.first + idx];
    const tp_replay_port_t pt = a.port[p];
    double* lds = lds_all[wave];
    const int k = pt.k, D = a.D, R = a.R;
    const size_t ld = (size_t)a.ld;
    double* ret = a.ret + (size_t)p * (size_t)D;
    double* turn = a.turnover + (size_t)p * (size_t)R;
    double* met = a.metrics + (size_t)p * (size_t)R * TP_REPLAY_METRICS;
    const double* wts = a.weights + pt.w_off;
    const int* ucols = a.cols + pt.u_off;
    const double* ucaps = a.caps + pt.u_off;
    const int* prev = a.prev_slot + pt.m_off;
    const int* next = a.next_slot + pt.m_off;
    const double nan = __builtin_nan("");
    const double inf = __builtin_inf();
    const double cost_frac = pt.cost / 10000.0;

    // FED: the cursor into the portfolio's patches [pq, pend) and the rebalancing date of the patch under it (R: none left)
    int pq = 0, pend = 0, pnext = 0;
    long long src_off = 0, src_stride = 0, st_off = 0, st_stride = 0;
    double w_scale = 1.0;
    if (FED) {
        pq = uniform(pt.patch_first);
        pend = uniform(pt.patch_end);
        pnext = pq < pend ? uniform(a.patch_date[pq]) : a.R;
        src_off = uniform(pt.w_off); src_stride = uniform(pt.w_stride);
        st_off = uniform(pt.s_off); st_stride = uniform(pt.s_stride);
        w_scale = uniform(pt.w_scale);
    }
    // the row of rebalancing date j, the factor on it (raw: none) and whether its source entry is flagged
    const double* wrow = wts;
    bool raw = true;
    int bad = 0;
    auto resolve = [&](int j) {
        const bool patched = pnext == j;
        const double* src_row = a.weights + (src_off + (long long)j * src_stride);
        const double* patch_row = a.patch_rows + (long long)pq * a.patch_ld;
        wrow = patched ? patch_row : src_row;
        raw = patched || w_scale == 1.0;
        const int st = uniform(a.src_status[st_off + (long long)j * st_stride]);
        bad = patched ? 0 : st;
    };

    double w[SPL], rn[SPL];
    int col[SPL], cnext[SPL];
#pragma unroll
    for (int s = 0; s < SPL; ++s) {
        const int i = s * 64 + lane;
        w[s] = 0.0; rn[s] = 0.0; col[s] = 0;
        cnext[s] = i < k ? ucols[i] : 0;      // the universe of rebalancing date 0
    }
    if (lane == 0) { a.status[p] = 0; a.bad_day[p] = -1; }

    int jn = 0;                               // the next rebalancing date and its trading day (D: there is none)
    int reb_next = 0;
    double rf_next = 0.0;                     // rf[d + 1], requested a day ahead like the returns
    for (int d = 0; d < D; ++d) {
        const bool reb = reb_next == d;
        const double rf = rf_next;
        if (d + 1 < D) rf_next = a.rf[d + 1];
        double r[SPL];
#pragma unroll
        for (int s = 0; s < SPL; ++s) r[s] = rn[s];
        if (d + 1 < D) {
            const double* row = a.S + (size_t)(d + 1) * ld;
#pragma unroll
            for (int s = 0; s < SPL; ++s)
                if (s * 64 + lane < k) rn[s] = row[reb ? cnext[s] : col[s]];
        }
        double an[SPL], cp[SPL];
        int ps[SPL], ns[SPL];
#pragma unroll
        for (int s = 0; s < SPL; ++s) { an[s] = 0.0; cp[s] = 0.0; ps[s] = -1; ns[s] = 0; }
        if (EARLY && reb) {
            if (FED) resolve(jn);
#pragma unroll
            for (int s = 0; s < SPL; ++s) {
                const int i = s * 64 + lane;
                if (i < k) {
                    if (FED) {
                        const double x = wrow[i];
                        an[s] = raw ? x : w_scale * x;
                    } else {
                        an[s] = wts[(long long)jn * pt.w_stride + i];
                    }
                    cp[s] = ucaps[(long long)jn * pt.u_stride + i];
                    if (jn > 0) {
                        ps[s] = prev[(long long)jn * k + i];
                        ns[s] = next[(long long)(jn - 1) * k + i];
                    }
                }
            }
        }

        double rd = nan;
        if (d > 0) {
            // mark to market and drift (ref:1137-1159)
            double dr[SPL];
            double v[3] = {0.0, 0.0, 0.0};
#pragma unroll
            for (int s = 0; s < SPL; ++s) {
                dr[s] = 0.0;
                if (s * 64 + lane < k) {
                    const double wv = w[s];
                    const double x = r[s] * wv;
                    dr[s] = wv * (1 + r[s]);
                    if (!is_nan(wv)) v[0] += wv;
                    if (!is_nan(x)) v[1] += x;
                    if (!is_nan(dr[s])) v[2] += dr[s];
                }
            }
            wave_sums(v);
            const double cash = 1 - v[0];
            rd = v[1] + cash * rf;
            const double cash_after = cash * (1 + rf);
            const double total = v[2] + cash_after;
            double part = 0.0;
#pragma unroll
            for (int s = 0; s < SPL; ++s) {
                if (s * 64 + lane < k) {
                    w[s] = dr[s] / total;
                    part += w[s];
                }
            }
            const double sum_w = wave_sum(part);                 // plain sum: a NaN never trips the check, as on the host
            const int tripped = __builtin_amdgcn_readfirstlane((int)(fabs((sum_w + cash_after / total) - 1) > 1e-5));
            if (tripped) {
                if (lane == 0) { a.status[p] = TP_REPLAY_KSTATUS_SUM_CHECK; a.bad_day[p] = d; }
                for (int t = d + lane; t < D; t += 64) ret[t] = nan;
                for (int t = jn + lane; t < R; t += 64) {
                    turn[t] = nan;
                    for (int c = 0; c < TP_REPLAY_METRICS; ++c) met[(size_t)t * TP_REPLAY_METRICS + c] = nan;
                }
                break;
            }
        }

        if (reb) {
            if (FED && !EARLY) resolve(jn);
            if (FED && bad != 0) {                                // the source flagged this row: the exit of the sum check
                if (lane == 0) { a.status[p] = TP_REPLAY_KSTATUS_BAD_WEIGHTS; a.bad_day[p] = d; }
                for (int t = d + lane; t < D; t += 64) ret[t] = nan;
                for (int t = jn + lane; t < R; t += 64) {
                    turn[t] = nan;
                    for (int c = 0; c < TP_REPLAY_METRICS; ++c) met[(size_t)t * TP_REPLAY_METRICS + c] = nan;
                }
                break;
            }
            if (!EARLY) {
#pragma unroll
                for (int s = 0; s < SPL; ++s) {
                    const int i = s * 64 + lane;
                    if (i < k) {
                        if (FED) {
                            const double x = wrow[i];
                            an[s] = raw ? x : w_scale * x;
                        } else {
                            an[s] = wts[(long long)jn * pt.w_stride + i];
                        }
                        if (jn > 0) {
                            ps[s] = prev[(long long)jn * k + i];
                            ns[s] = next[(long long)(jn - 1) * k + i];
                        }
                    }
                }
            }
            // sums of the new weights; with a portfolio before them, the turnover (ref:1054-1075)
            // v: nansum(caps), count > 0, count < 0, sum > 0, sum < 0, nansum(after), nansum(before), traded
            double v[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            double mx = -inf, mn = inf;
            if (jn > 0) {
#pragma unroll
                for (int s = 0; s < SPL; ++s) {
                    const int i = s * 64 + lane;
                    if (i < k) lds[i] = nan_to_zero(w[s]);
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            }
#pragma unroll
            for (int s = 0; s < SPL; ++s) {
                const int i = s * 64 + lane;
                if (i < k) {
                    const double x = an[s];
                    if (x > 0) { v[1] += 1.0; v[3] += x; mx = x > mx ? x : mx; }
                    if (x < 0) { v[2] += 1.0; v[4] += x; mn = x < mn ? x : mn; }
                    if (!is_nan(x)) v[5] += x;
                    if (jn > 0) {
                        const double b_own = nan_to_zero(w[s]);
                        v[6] += b_own;
                        const int q = ps[s];
                        const double b = (q >= 0 && q < k) ? lds[q] : 0.0;
                        v[7] += fabs(b - nan_to_zero(x));
                        if (ns[s] < 0) v[7] += fabs(b_own);
                    }
                }
            }
            if (!EARLY) {
#pragma unroll
                for (int s = 0; s < SPL; ++s) {
                    const int i = s * 64 + lane;
                    if (i < k) cp[s] = ucaps[(long long)jn * pt.u_stride + i];
                }
            }
#pragma unroll
            for (int s = 0; s < SPL; ++s)
                if (s * 64 + lane < k && !is_nan(cp[s])) v[0] += cp[s];
            wave_sums(v);
            mx = wave_max(mx);
            mn = wave_min(mn);
            // distance to the value-weighted portfolio of the same universe (ref:692-695, 1100-1104)
            double u[2] = {0.0, 0.0};
#pragma unroll
            for (int s = 0; s < SPL; ++s) {
                if (s * 64 + lane < k) {
                    const double x = fabs(an[s] * pt.scaling - cp[s] / v[0]);
                    if (!is_nan(x)) { u[0] += x; u[1] += 1.0; }
                }
            }
            wave_sums(u);
            double to = nan;
            if (jn > 0) {
                to = (v[7] + fabs(v[6] - v[5])) / 2;
                rd -= cost_frac * to;                             // ref:1212
            }
            if (lane == 0) {
                double* m = met + (size_t)jn * TP_REPLAY_METRICS;
                m[0] = v[1] > 0 ? mx : nan;
                m[1] = v[2] > 0 ? mn : nan;
                m[2] = v[1] > 0 ? v[3] / v[1] : nan;
                m[3] = v[2] > 0 ? v[4] / v[2] : nan;
                m[4] = u[0] / u[1];
                turn[jn] = to;
            }
#pragma unroll
            for (int s = 0; s < SPL; ++s) {
                w[s] = an[s];
                col[s] = cnext[s];
            }
            if (FED && pnext == jn) {                             // this date was a patch: on to the portfolio's next one
                ++pq;
                pnext = pq < pend ? uniform(a.patch_date[pq]) : R;
            }
            ++jn;
            reb_next = jn < R ? a.reb_day[jn] : D;
            if (jn < R) {
#pragma unroll
                for (int s = 0; s < SPL; ++s) {
                    const int i = s * 64 + lane;
                    if (i < k) cnext[s] = ucols[(long long)jn * pt.u_stride + i];
                }
            }
        }
        if (lane == 0) ret[d] = rd;
    }
}

template <int SPL>
hipError_t launch_spl(const tp_replay_args_t& a, hipStream_t st) {
    const int grid = (a.count + TP_REPLAY_WAVES - 1) / TP_REPLAY_WAVES;
    if (a.src_status) hipLaunchKernelGGL((replay_kernel<SPL, true>), dim3(grid), dim3(64 * TP_REPLAY_WAVES), 0, st, a);
    else hipLaunchKernelGGL((replay_kernel<SPL, false>), dim3(grid), dim3(64 * TP_REPLAY_WAVES), 0, st, a);
    return hipGetLastError();
}

}  // namespace

int tp_replay_slots_per_lane(int k) {
    int spl = 1;
    while (spl * 64 < k) spl *= 2;
    return spl;
}

hipError_t tp_replay_launch(const tp_replay_args_t& a, int spl, hipStream_t st) {
    if (a.count <= 0) return hipSuccess;
    switch (spl) {
        case 1: return launch_spl<1>(a, st);
        case 2: return launch_spl<2>(a, st);
        case 4: return launch_spl<4>(a, st);
        case 8: return launch_spl<8>(a, st);
        case 16: return launch_spl<16>(a, st);
        case 32: return launch_spl<32>(a, st);
    }
    return hipErrorInvalidValue;
}
