// replay_summary.hip - the performance statistics of a replay's daily returns (backtest_replay.hip) at MANY trading costs, read
// where the replay left them: ONE WAVEFRONT PER (PORTFOLIO, COST).  The waves of a workgroup take costs of the same portfolio,
// so its row of returns comes from HBM once.  A cost never touches the holdings: it enters a replay only through
// ret[reb_day[j]] -= cost / 10000 * turnover[j] (ref:1212), so the net returns of every cost follow from one replay at cost 0.
//
// The series (include/tangency_posterior.h has the definitions): the net return x, the excess return e = x - rf_excess, and
// `adjust_returns` (ref:46-72) applied to each - a from x, b from e.  Days go through in tiles of 64 consecutive days, lane l
// takes day base + l.  The compounded wealth W_d = prod (1 + a_d) is a six-step inclusive scan across the wave times the carry
// of the tile before; a second scan forms the running peak.  The first day under -100 % (and, for a, under -99 %, ref:27-33)
// is found with a ballot, which is wave-uniform; the tile that holds it is formed again with the adjusted values.  Every sum is
// a lane-local partial in tile order followed by the replay's fixed 64-lane tree: bit-reproducible from run to run and
// independent of the other portfolios and costs of the launch.  A second pass over the row forms the centred moments.
// Compiled with -ffp-contract=off: one rounding per operation.  No barrier, no spin; every loop is bounded by D or R.
#include "replay_summary.h"
#include "replay_wave_prims.h"

namespace {

__device__ __forceinline__ bool finite(double x) { return __builtin_fabs(x) < __builtin_inf(); }

// inclusive scans over the 64 lanes, six fixed steps; lanes below the step keep their value
__device__ __forceinline__ double scan_product(double v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const double t = __shfl_up(v, o, 64);
        v = lane >= o ? v * t : v;
    }
    return v;
}

__device__ __forceinline__ double scan_max(double v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const double t = __shfl_up(v, o, 64);
        v = lane >= o ? pick_max(v, t) : v;
    }
    return v;
}

// One series' `adjust_returns` state: the wealth after the last tile, the adjusted day (-1: none yet) and its value.
struct Adjust {
    double carry = 1.0;
    long long day = -1;
    double value = 0.0;
};

// A tile of one series: `v` comes in as the unadjusted value of the lane's day (0 on a lane past the end) and leaves adjusted;
// returns the wealth W of the lane's day.  All 64 lanes are active; `s` is wave-uniform before and after.
__device__ __forceinline__ double adjust_tile(Adjust& s, double& v, long long base, int lane, bool valid) {
    if (s.day >= 0) v = 0.0;                                  // every day after the adjusted one
    double w = s.carry * scan_product(1 + v, lane);
    if (s.day < 0) {
        const unsigned long long under = __ballot(valid && w - 1 < -1);
        if (under != 0) {
            const int i = uniform((int)__builtin_ctzll(under));
            const double before = uniform(readlane_d(w, i > 0 ? i - 1 : 0));
            const double prev = i > 0 ? before : s.carry;     // W of the day before
            s.day = base + i;
            s.value = s.day == 1 ? -1.0 : 0.000001 / (prev - 1) - 1;   // ref:59-66, as written
            v = lane < i ? v : (lane == i ? s.value : 0.0);
            w = s.carry * scan_product(1 + v, lane);
        }
    }
    s.carry = uniform(readlane_d(w, 63));                     // (a lane past the end holds the last day's)
    return w;
}

// the value of day d in a series whose adjustment is known (second pass)
__device__ __forceinline__ double adjusted(const Adjust& s, double raw, long long d) {
    return (s.day < 0 || d < s.day) ? raw : (d == s.day ? s.value : 0.0);
}

__global__ __launch_bounds__(64 * TP_SUMMARY_WAVES) void summary_kernel(const tp_summary_args_t a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int p = blockIdx.x;
    const int c = blockIdx.y * TP_SUMMARY_WAVES + wave;
    if (c >= a.C) return;                                     // (a whole wave; the waves of a workgroup never meet)
    const long long D = a.D;
    const int R = a.R;
    const double* ret = a.ret + (size_t)p * (size_t)D;
    const double* turn = a.turnover + (size_t)p * (size_t)R;
    double* out = a.stats + ((size_t)p * (size_t)a.C + (size_t)c) * TP_SUMMARY_NSTATS;
    int* out_status = a.status + ((size_t)p * (size_t)a.C + (size_t)c);
    const double nan = __builtin_nan("");
    const double inf = __builtin_inf();

    if (uniform(a.rstatus[p]) != 0) {                         // the replay gave this portfolio up
        if (lane < TP_SUMMARY_NSTATS) out[lane] = lane < 28 ? nan : 0.0;
        if (lane == 0) *out_status = TP_SUMMARY_KSTATUS_NO_REPLAY;
        return;
    }
    const double cost_frac = uniform(a.cost_bp[c]) / 10000.0;
    const double n = (double)(D - 1);

    // the lane's day of a tile: net and excess return as §1 of the header defines them
    auto load = [&](long long d, bool valid, double& x, double& e) {
        x = 0.0; e = 0.0;
        if (valid) {
            x = ret[d];
            const int j = a.day_date[d];
            if (j >= 1) x = x - cost_frac * turn[j];          // a selection: no turnover reaches any other day
            e = x - a.rf_excess[d];
        }
    };

    // ---- first pass: adjustment, insolvency, wealth, drawdown, plain sums
    Adjust sa, sb;
    long long ins = -1;                                       // first day with W - 1 < -0.99 on a
    double peak = -inf;
    // sums: a, wins, n wins, losses, n losses, |a| > 1e-7, n of them, n before insolvency, a before it, b, b^2 over b < 0
    double v[13] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    double best = -inf, worst = inf, worst_pre = inf, mdd = inf;
    bool bad = false;
    for (long long base = 1; base < D; base += 64) {
        const long long d = base + lane;
        const bool valid = d < D;
        double av, bv;
        load(d, valid, av, bv);
        const double w = adjust_tile(sa, av, base, lane, valid);
        (void)adjust_tile(sb, bv, base, lane, valid);
        if (ins < 0) {
            const unsigned long long under = __ballot(valid && w - 1 < -0.99);
            if (under != 0) ins = base + uniform((int)__builtin_ctzll(under));
        }
        const double pk = pick_max(scan_max(w, lane), peak);
        peak = uniform(readlane_d(pk, 63));
        if (valid) {
            bad = bad || !finite(av) || !finite(bv);
            mdd = pick_min(mdd, w / pk - 1);
            v[0] += av;
            best = pick_max(best, av);
            worst = pick_min(worst, av);
            if (av > 0) { v[1] += av; v[2] += 1.0; }
            if (av < 0) { v[3] += av; v[4] += 1.0; }
            if (__builtin_fabs(av) > 1e-7) { v[5] += av; v[6] += 1.0; }
            if (ins < 0 || d < ins) { v[7] += 1.0; v[8] += av; worst_pre = pick_min(worst_pre, av); }
            v[9] += bv;
            if (bv < 0) v[10] += bv * bv;
        }
    }
    // the turnover up to the insolvency (ref:696)
    for (int t = 1 + lane; t < R; t += 64)
        if (ins < 0 || a.reb_day[t] <= ins) { v[11] += turn[t]; v[12] += 1.0; }
    wave_sums(v);
    best = wave_max(best);
    worst = wave_min(worst);
    worst_pre = wave_min(worst_pre);
    mdd = wave_min(mdd);
    const bool nonfinite = __ballot(bad) != 0;
    const double n_pre = v[7];
    const double mean = v[0] / n, mean_pre = v[8] / n_pre, mean_e = v[9] / n;

    // ---- second pass: centred moments
    double q[5] = {0.0, 0.0, 0.0, 0.0, 0.0};                  // (a - mean)^2, the same before the insolvency, (b - mean_e)^2, ^3, ^4
    for (long long base = 1; base < D; base += 64) {
        const long long d = base + lane;
        const bool valid = d < D;
        double x, e;
        load(d, valid, x, e);
        if (valid) {
            const double av = adjusted(sa, x, d), bv = adjusted(sb, e, d);
            const double ca = av - mean;
            q[0] += ca * ca;
            if (ins < 0 || d < ins) {
                const double cp = av - mean_pre;
                q[1] += cp * cp;
            }
            const double cb = bv - mean_e, cb2 = cb * cb;
            q[2] += cb2;
            q[3] += cb2 * cb;
            q[4] += cb2 * cb2;
        }
    }
    wave_sums(q);

    if (lane == 0) {
        double r[TP_SUMMARY_NSTATS];
        r[0] = n;
        r[1] = (double)sa.day;
        r[2] = (double)ins;
        r[3] = sa.carry - 1;
        r[4] = mean;
        r[5] = n >= 2 ? sqrt(q[0] / (n - 1)) : nan;
        r[6] = mdd < inf ? mdd : nan;                         // no day has a drawdown: the peak is 0 (day 1 was adjusted), 0 / 0
        r[7] = best;
        r[8] = worst;
        r[9] = v[1]; r[10] = v[2]; r[11] = v[3]; r[12] = v[4];
        r[13] = n_pre;
        r[14] = mean_pre;
        r[15] = n_pre >= 2 ? sqrt(q[1] / (n_pre - 1)) : nan;
        r[16] = n_pre >= 1 ? worst_pre : nan;
        r[17] = v[5]; r[18] = v[6];
        r[19] = (double)sb.day;
        r[20] = mean_e;
        r[21] = n >= 2 ? sqrt(q[2] / (n - 1)) : nan;
        r[22] = q[2] / n; r[23] = q[3] / n; r[24] = q[4] / n;
        r[25] = v[10] / n;
        r[26] = v[11]; r[27] = v[12];
#pragma unroll
        for (int i = 0; i < TP_SUMMARY_NSTATS; ++i) {
            const bool kept = i == 0 || i == 1 || i == 2 || i == 19;
            out[i] = i >= 28 ? 0.0 : (nonfinite && !kept ? nan : r[i]);
        }
        *out_status = nonfinite ? TP_SUMMARY_KSTATUS_NONFINITE : 0;
    }
}

}  // namespace

hipError_t tp_summary_launch(const tp_summary_args_t& a, hipStream_t st) {
    if (a.P <= 0) return hipSuccess;
    const dim3 grid((unsigned)a.P, (unsigned)((a.C + TP_SUMMARY_WAVES - 1) / TP_SUMMARY_WAVES));
    hipLaunchKernelGGL(summary_kernel, grid, dim3(64 * TP_SUMMARY_WAVES), 0, st, a);
    return hipGetLastError();
}
