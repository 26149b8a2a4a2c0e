// sweep_finish.hip - the Greyserman and Jorion weights from the solutions of a solve sweep (S shifts, right-hand sides [t, 1]),
// read where the sweep left them: ONE WAVEFRONT PER (WINDOW, GROUP OF TP_FINISH_DRAWS_PER_WAVE CONSECUTIVE SHIFTS).  Both
// finishes are three dot products per (window, shift) - 1'u_one, 1'u_t, t'u_t -, a dozen scalar operations that give the
// coefficients of the two solution rows, and the mean over the shifts of that combination (include/tangency_posterior.h has
// the definitions, one rounding per operation).
//
// Lane l owns the columns l, l + 64, ... (NS slots, a template parameter: 1, 2, 3, 4, 8, 16 or 32, the smallest that covers k).
// Per shift the lane's slots of the two rows are loaded (8-byte loads: a row is not 16-byte aligned when k is odd), the three
// sums are a lane-local partial in slot order followed by the replay's fixed 64-lane tree (replay_wave_prims.h), the scalar
// algebra runs alike in every lane, and the combination is added to the lane's accumulators.  The rows of the next shift are
// requested before the sums of the current one.  A group's partial sums go to part [W x NG x k]; the second launch adds a
// window's NG partials in ascending order, divides by S and writes the weights and the status.
// The grouping and every order of summation depend on (k, S) only: a window's result is the same bit for bit whatever W, its
// position and the sub-ranges of the sweep that fed it.  No atomics, no barrier, no spin; every loop is bounded by S, k or NG.
// Compiled with -ffp-contract=off: one rounding per operation.
#include "sweep_finish.h"
#include "replay_wave_prims.h"

namespace {

__device__ __forceinline__ bool finite(double x) { return __builtin_fabs(x) < __builtin_inf(); }

// the lane's slots of the two solution rows of (window, shift) pair `e`; 0 past column k
template <int NS>
__device__ __forceinline__ void load_rows(const double* x, size_t e, int k, int lane, double (&ut)[NS], double (&uo)[NS]) {
    const double* r0 = x + e * 2 * (size_t)k;
    const double* r1 = r0 + k;
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        const int j = lane + 64 * i;
        ut[i] = j < k ? r0[j] : 0.0;
        uo[i] = j < k ? r1[j] : 0.0;
    }
}

template <int MODE, int NS>
__global__ __launch_bounds__(64) void finish_group_kernel(const tp_finish_args_t a) {
    const int lane = threadIdx.x;
    const int S = a.S, k = a.k;
    const int NG = (S + TP_FINISH_DRAWS_PER_WAVE - 1) / TP_FINISH_DRAWS_PER_WAVE;
    const int w = blockIdx.x / NG, g = blockIdx.x - w * NG;
    const int s_first = g * TP_FINISH_DRAWS_PER_WAVE;
    // (Jorion: S = 1, one shift per wave - stated so that its form carries no registers for a next shift)
    const int s_end = MODE == TP_FINISH_KMODE_JORION ? s_first + 1
                      : (s_first + TP_FINISH_DRAWS_PER_WAVE < S ? s_first + TP_FINISH_DRAWS_PER_WAVE : S);
    const size_t e0 = (size_t)w * (size_t)S;
    const double nan = __builtin_nan("");

    double t[NS], acc[NS];
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        const int j = lane + 64 * i;
        t[i] = j < k ? a.t[(size_t)w * (size_t)k + j] : 0.0;
        acc[i] = 0.0;
    }
    const double n = a.n[w];
    const double N = (double)k;
    // wave-uniform scalars of the window
    double c = 0.0, kappa = 0.0, kJ = 0.0;
    if (MODE == TP_FINISH_KMODE_GREYSERMAN) {
        kappa = a.kappa[w];
        c = tp_finish_greyserman_scale(a.gamma, N, n);
    } else {
        kJ = (((n - N) - 2) * (n - 1)) / n;
    }

    double ut[NS], uo[NS], ut_next[NS], uo_next[NS];
    double xi = 0.0, eta = 0.0, xi_next = 0.0, eta_next = 0.0;
    load_rows<NS>(a.x, e0 + s_first, k, lane, ut, uo);
    int st = a.xstatus[e0 + s_first];
    if (MODE == TP_FINISH_KMODE_GREYSERMAN) { xi = a.hyper[2 * (e0 + s_first)]; eta = a.hyper[2 * (e0 + s_first) + 1]; }
    int first_bad = 0;
    for (int s = s_first; s < s_end; ++s) {
        int st_next = 0;
        if (s + 1 < s_end) {                                  // the next shift's rows, ahead of this shift's reductions
            load_rows<NS>(a.x, e0 + s + 1, k, lane, ut_next, uo_next);
            st_next = a.xstatus[e0 + s + 1];
            if (MODE == TP_FINISH_KMODE_GREYSERMAN) { xi_next = a.hyper[2 * (e0 + s + 1)]; eta_next = a.hyper[2 * (e0 + s + 1) + 1]; }
        }
        double* aux = a.aux + (e0 + s) * 4;
        if (uniform(st) != 0) {                               // the sweep gave this shift up: its rows are not read as numbers
            if (first_bad == 0) first_bad = uniform(st);
            if (lane < 4) aux[lane] = nan;
        } else {
            double v[3] = {0.0, 0.0, 0.0};                    // 1'u_one, 1'u_t, t'u_t
#pragma unroll
            for (int i = 0; i < NS; ++i) {
                v[0] += uo[i];
                v[1] += ut[i];
                v[2] += t[i] * ut[i];
            }
            wave_sums(v);
            const double s1 = v[0], s2 = v[1], s3 = v[2];
            if (MODE == TP_FINISH_KMODE_GREYSERMAN) {
                const tp_finish_coeffs_t f = tp_finish_greyserman_coeffs(s1, s2, s3, n, kappa, xi, eta, c);
#pragma unroll
                for (int i = 0; i < NS; ++i) acc[i] += f.cA * uo[i] - f.cB * ut[i];
                if (lane == 0) { aux[0] = s1; aux[1] = s2; aux[2] = s3; aux[3] = f.det; }
            } else {
                const double T = n;
                const double sbb = kJ * s1, sab = (kJ * s2) / T, saa = (kJ * s3) / (T * T);
                const double mug = sab / sbb;
                const double q = (saa - (2 * mug) * sab) + (mug * mug) * sbb;
                const double lam = (N + 2) / q;
                const double vv = (N + 2) / ((N + 2) + T * q);
                const double alpha = 1 + 1 / (T + lam);
                const double beta = (lam / (T * ((T + 1) + lam))) / sbb;
                const double gsum = (1 - vv) * sab + (vv * mug) * sbb;
                const double cT = (((1 - vv) * kJ) / T) / alpha;
                const double cO = ((vv * mug) * kJ) / alpha;
                const double cS = (((beta / (alpha * alpha)) * kJ) * gsum) / (1 + (beta / alpha) * sbb);
#pragma unroll
                for (int i = 0; i < NS; ++i) acc[i] += ((cT * ut[i] + cO * uo[i]) - cS * uo[i]) / a.gamma;
                if (lane == 0) { aux[0] = s1; aux[1] = s2; aux[2] = s3; aux[3] = q; }
            }
        }
        if (s + 1 < s_end) {
#pragma unroll
            for (int i = 0; i < NS; ++i) { ut[i] = ut_next[i]; uo[i] = uo_next[i]; }
            st = st_next; xi = xi_next; eta = eta_next;
        }
    }
    double* part = a.part + (size_t)blockIdx.x * (size_t)k;
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        const int j = lane + 64 * i;
        if (j < k) part[j] = acc[i];
    }
    if (lane == 0) a.gstatus[blockIdx.x] = first_bad;
}

// One wavefront per window: the NG partial sums of every column in ascending order, the mean, the status.
__global__ __launch_bounds__(64) void finish_window_kernel(const tp_finish_args_t a) {
    const int lane = threadIdx.x;
    const int S = a.S, k = a.k;
    const int NG = (S + TP_FINISH_DRAWS_PER_WAVE - 1) / TP_FINISH_DRAWS_PER_WAVE;
    const int w = blockIdx.x;
    const double* part = a.part + (size_t)w * (size_t)NG * (size_t)k;
    double* out = a.weights + (size_t)w * (size_t)k;
    int bad = 0;
    for (int g = 0; g < NG; ++g) {                            // (every lane reads the same word)
        const int gs = a.gstatus[(size_t)w * NG + g];
        if (bad == 0) bad = gs;
    }
    bad = uniform(bad);
    bool nonfinite = false;
    for (int j = lane; j < k; j += 64) {
        double sum = part[j];
        for (int g = 1; g < NG; ++g) sum += part[(size_t)g * (size_t)k + j];
        const double wj = bad != 0 ? __builtin_nan("") : sum / (double)S;
        nonfinite = nonfinite || !finite(wj);
        out[j] = wj;
    }
    const bool any = __ballot(nonfinite) != 0;
    if (lane == 0) a.status[w] = bad != 0 ? bad : (any ? TP_FINISH_KSTATUS_NONFINITE : 0);
}

template <int MODE>
hipError_t launch_groups(const tp_finish_args_t& a, unsigned blocks, hipStream_t st) {
    const int slots = (a.k + 63) / 64;
#define TP_FINISH_CASE(NS) \
    if (slots <= NS) { hipLaunchKernelGGL((finish_group_kernel<MODE, NS>), dim3(blocks), dim3(64), 0, st, a); return hipGetLastError(); }
    TP_FINISH_CASE(1)
    TP_FINISH_CASE(2)
    TP_FINISH_CASE(3)
    TP_FINISH_CASE(4)
    TP_FINISH_CASE(8)
    TP_FINISH_CASE(16)
    TP_FINISH_CASE(TP_FINISH_MAX_SLOTS)
#undef TP_FINISH_CASE
    return hipErrorInvalidValue;
}

}  // namespace

hipError_t tp_finish_launch(const tp_finish_args_t& a, hipStream_t st) {
    if (a.W <= 0) return hipSuccess;
    const long long NG = (a.S + TP_FINISH_DRAWS_PER_WAVE - 1) / TP_FINISH_DRAWS_PER_WAVE;
    const long long blocks = (long long)a.W * NG;
    if (a.S < 1 || a.k < 1 || a.k > 64 * TP_FINISH_MAX_SLOTS || blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    const hipError_t e = a.mode == TP_FINISH_KMODE_JORION ? launch_groups<TP_FINISH_KMODE_JORION>(a, (unsigned)blocks, st)
                                                          : launch_groups<TP_FINISH_KMODE_GREYSERMAN>(a, (unsigned)blocks, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(finish_window_kernel, dim3((unsigned)a.W), dim3(64), 0, st, a);
    return hipGetLastError();
}
