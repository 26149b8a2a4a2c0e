// posterior_spectral.hip - spectral ridge sweep (tp_batch_spectral_greyserman): the Greyserman weights of S ridge shifts per
// window from ONE eigendecomposition.  Every shift of a window is a multiple of the identity, so all S matrices M + d_s I share
// the eigenvectors of M = V diag(lambda) V':
//
//     (M + d I)^-1 b = V diag(1 / (lambda_j + d)) V'b ,
//
// and the finish's three sums, its rank-two algebra and the mean over the draws can all be taken in the eigenbasis.  One product
// V w^ per window gives the weights.  Three kernels per sub-range of windows:
//
// spectral_jacobi_kernel - ONE 256-THREAD WORKGROUP PER WINDOW.  Two-sided cyclic Jacobi.  The working matrix is the packed
// lower triangle of posterior_sweep_solve.h in LDS (column c holds rows c .. k + 1 at sweep_off(c, k + 2)); rows k and k + 1
// are t^ = V't and o^ = V'1, which start as t and the ones vector and take every COLUMN rotation.  V is accumulated in global
// memory, column-major, from the identity: a rotation touches two contiguous columns.
//   A sweep is the m - 1 rounds of a round-robin tournament over m = 2 ceil(k / 2) players (rr_pair: a function of k only); a
//   round's m / 2 pairs are disjoint.  Round, step 1: thread u < m / 2 reads (a_pp, a_qq, a_pq) of its pair - no other pair of
//   the round touches them -, decides, forms (c, s), writes the pair's own 2 x 2 block and leaves (c, s) in LDS.  A pair with
//   |a_pq| <= 2^-53 max(sqrt(|a_pp a_qq|), a_max), a_max = max_i |M_ii| of the input, is skipped; after a rotation a_pq is
//   exactly 0.  Step 2: the 2 x 2 block between two pairs u < v is owned by one thread - columns by pair v's rotation, then rows
//   by pair u's -, the extra rows and the columns of V by one thread per element pair.  No element is written by two threads
//   in a step, and every element's operations depend on k and the data only: the result is the same bits from run to run.
//   Convergence: a whole sweep without a rotation; at most TP_SPECTRAL_KMAX_SWEEPS sweeps.
//   Two workgroup barriers per round (one when the round rotated nothing), each reached by every thread: the decisions they
//   carry (__syncthreads_or) are uniform.  Nothing spins, no flags between workgroups, no atomics; every loop is bounded by k
//   and the cap.
// spectral_group_kernel - ONE WAVEFRONT PER (WINDOW, TP_FINISH_DRAWS_PER_WAVE CONSECUTIVE SHIFTS), the shape of
//   finish_group_kernel: lane l owns the eigen-indices l, l + 64, l + 128.
// spectral_window_kernel - ONE WAVEFRONT PER WINDOW: the groups' partial sums in ascending order, the mean, w = V w^.
// Compiled with -ffp-contract=off: one rounding per operation.
#include "posterior_spectral.h"
#include "posterior_sweep_solve.h"
#include "sweep_finish.h"
#include "replay_wave_prims.h"

namespace {

constexpr int SPEC_MAX_PAIRS = (SWEEP_MAX_K + 1) / 2;
constexpr int SPEC_SLOTS = 3;            // eigen-indices per lane: k <= 64 * 3
constexpr double SPEC_EPS = 0x1p-53;

__device__ __forceinline__ bool finite(double x) { return __builtin_fabs(x) < __builtin_inf(); }

// Pair u of round r of the tournament over m players (m even, 0 <= r < m - 1, 0 <= u < m / 2): player m - 1 stays, the others
// go round.  p < q; a q >= k (k odd: the player m - 1 = k) means p sits the round out.
__device__ __forceinline__ void rr_pair(int u, int r, int m, int& p, int& q) {
    int a, b;
    if (u == 0) {
        a = m - 1; b = r;
    } else {
        a = r + u; if (a >= m - 1) a -= m - 1;
        b = r - u; if (b < 0) b += m - 1;
    }
    p = a < b ? a : b;
    q = a < b ? b : a;
}

__global__ void __launch_bounds__(SWEEP_THREADS) spectral_jacobi_kernel(const tp_spectral_args_t A) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    __shared__ double rot_c[SPEC_MAX_PAIRS], rot_s[SPEC_MAX_PAIRS];
    __shared__ int rot_pq[SPEC_MAX_PAIRS];                  // p | q << 8 | (1 << 16 when the pair rotates)
    const int tid = threadIdx.x;
    const int k = A.k, H = k + 2;
    const long long wl = blockIdx.x;
    if (wl >= A.w_count) return;
    const long long w = A.w_first + wl;
    const double* __restrict__ M = A.post + wl * (long long)k * k;
    const double* __restrict__ t = A.t + w * (long long)k;
    double* V = A.V + (A.v_first + wl) * (long long)k * k;
    auto off = [H](int c) { return sweep_off(c, H); };
    // element (x, y), x != y, of the symmetric matrix in the lower triangle
    auto at = [H](int x, int y) { return x > y ? sweep_off(y, H) + (x - y) : sweep_off(x, H) + (y - x); };

    // ---- load: column c of the lower triangle = row c of the symmetric M from the diagonal on (coalesced), t and 1 below it
    bool bad = false;
    {
        const int tx = tid & (SWEEP_TX - 1), ty = tid / SWEEP_TX;
        for (int c = ty; c < k; c += SWEEP_TY) {
            double* col = lds + off(c) - c;
            for (int i = c + tx; i < k; i += SWEEP_TX) {
                const double v = M[(long long)c * k + i];
                col[i] = v;
                bad = bad || !finite(v);
            }
        }
        for (int c = tid; c < k; c += SWEEP_THREADS) {
            const double v = t[c];
            lds[off(c) + (k - c)] = v;
            lds[off(c) + (k + 1 - c)] = 1.0;
            bad = bad || !finite(v);
        }
        for (int e = tid; e < k * k; e += SWEEP_THREADS) V[e] = e % (k + 1) == 0 ? 1.0 : 0.0;
    }
    const bool nonfinite = __syncthreads_or(bad ? 1 : 0) != 0;
    double amax = 0.0;
    for (int j = 0; j < k; ++j) amax = pick_max(amax, __builtin_fabs(lds[off(j)]));   // (every thread reads the same words)

    const int m = (k + 1) & ~1, NP = m / 2;
    const int lane = tid & 63, wv = tid >> 6;
    const int bx = tid & 15, by = tid >> 4;
    int sweeps = 0;
    bool converged = false;
    if (!nonfinite) {
        for (int sweep = 0; sweep < TP_SPECTRAL_KMAX_SWEEPS; ++sweep) {
            bool rotated = false;
            for (int r = 0; r < m - 1; ++r) {
                // ---- step 1: the round's rotations, one thread per pair
                bool mine = false;
                if (tid < NP) {
                    int p, q;
                    rr_pair(tid, r, m, p, q);
                    double c = 1.0, s = 0.0;
                    if (q < k) {
                        const int ipp = off(p), iqq = off(q), ipq = ipp + (q - p);
                        const double app = lds[ipp], aqq = lds[iqq], apq = lds[ipq];
                        const double floor = SPEC_EPS * pick_max(__builtin_sqrt(__builtin_fabs(app * aqq)), amax);
                        if (__builtin_fabs(apq) > floor) {
                            const double theta = (aqq - app) / (2 * apq);
                            const double tt = (theta < 0 ? -1.0 : 1.0) / (__builtin_fabs(theta) + __builtin_sqrt(theta * theta + 1));
                            c = 1 / __builtin_sqrt(tt * tt + 1);
                            s = tt * c;
                            lds[ipp] = app - tt * apq;
                            lds[iqq] = aqq + tt * apq;
                            lds[ipq] = 0.0;
                            mine = true;
                        }
                    }
                    rot_c[tid] = c; rot_s[tid] = s;
                    rot_pq[tid] = p | (q << 8) | (mine ? 1 << 16 : 0);
                }
                rotated = rotated || mine;
                if (!__syncthreads_or(mine ? 1 : 0)) continue;      // (uniform: nobody reads rot_* of a round that rotated nothing)
                // ---- step 2a: the 2 x 2 blocks between the pairs u < v
                for (int u = by; u < NP; u += 16) {
                    const int pqu = rot_pq[u];
                    const int p1 = pqu & 255, q1 = (pqu >> 8) & 255;
                    const double c1 = rot_c[u], s1 = rot_s[u];
                    for (int v = u + 1 + bx; v < NP; v += 16) {
                        const int pqv = rot_pq[v];
                        if (((pqu | pqv) >> 16) == 0) continue;
                        const int p2 = pqv & 255, q2 = (pqv >> 8) & 255;
                        const double c2 = rot_c[v], s2 = rot_s[v];
                        const bool h1 = q1 < k, h2 = q2 < k;           // (a pair that sits out has no second index)
                        const int i00 = at(p1, p2), i01 = h2 ? at(p1, q2) : i00, i10 = h1 ? at(q1, p2) : i00,
                                  i11 = h1 && h2 ? at(q1, q2) : i00;
                        const double b00 = lds[i00], b01 = h2 ? lds[i01] : 0.0, b10 = h1 ? lds[i10] : 0.0,
                                     b11 = h1 && h2 ? lds[i11] : 0.0;
                        const double t00 = c2 * b00 - s2 * b01, t01 = s2 * b00 + c2 * b01;
                        const double t10 = c2 * b10 - s2 * b11, t11 = s2 * b10 + c2 * b11;
                        lds[i00] = c1 * t00 - s1 * t10;
                        if (h2) lds[i01] = c1 * t01 - s1 * t11;
                        if (h1) lds[i10] = s1 * t00 + c1 * t10;
                        if (h1 && h2) lds[i11] = s1 * t01 + c1 * t11;
                    }
                }
                // ---- step 2b: the rows t^ and o^
                for (int e = tid; e < 2 * NP; e += SWEEP_THREADS) {
                    const int u = e >> 1, row = k + (e & 1);
                    const int pq = rot_pq[u];
                    if ((pq >> 16) == 0) continue;
                    const int p = pq & 255, q = (pq >> 8) & 255;
                    const double c = rot_c[u], s = rot_s[u];
                    const int ip = off(p) + (row - p), iq = off(q) + (row - q);
                    const double ep = lds[ip], eq = lds[iq];
                    lds[ip] = c * ep - s * eq;
                    lds[iq] = s * ep + c * eq;
                }
                // ---- step 2c: the columns of V, one wavefront per pair
                for (int u = wv; u < NP; u += SWEEP_THREADS / 64) {
                    const int pq = rot_pq[u];
                    if ((pq >> 16) == 0) continue;
                    const int p = pq & 255, q = (pq >> 8) & 255;
                    const double c = rot_c[u], s = rot_s[u];
                    double* vp = V + (long long)p * k;
                    double* vq = V + (long long)q * k;
                    for (int i = lane; i < k; i += 64) {
                        const double xp = vp[i], xq = vq[i];
                        vp[i] = c * xp - s * xq;
                        vq[i] = s * xp + c * xq;
                    }
                }
                __syncthreads();
            }
            ++sweeps;
            if (!__syncthreads_or(rotated ? 1 : 0)) { converged = true; break; }
        }
    }
    for (int j = tid; j < k; j += SWEEP_THREADS) {
        A.lambda[w * k + j] = lds[off(j)];
        A.that[w * k + j] = lds[off(j) + (k - j)];
        A.ohat[w * k + j] = lds[off(j) + (k + 1 - j)];
    }
    if (tid == 0) {
        A.sweeps[w] = sweeps;
        A.jstatus[w] = nonfinite ? TP_KSTATUS_NONFINITE : converged ? TP_KSTATUS_OK : TP_SPECTRAL_KSTATUS_NO_CONVERGENCE;
    }
}

__global__ __launch_bounds__(64) void spectral_group_kernel(const tp_spectral_args_t a) {
    const int lane = threadIdx.x;
    const int S = a.S, k = a.k;
    const int NG = (S + TP_FINISH_DRAWS_PER_WAVE - 1) / TP_FINISH_DRAWS_PER_WAVE;
    const long long wl = blockIdx.x / NG;
    const int g = (int)(blockIdx.x - wl * NG);
    const long long w = a.w_first + wl;
    const int s_first = g * TP_FINISH_DRAWS_PER_WAVE;
    const int s_end = s_first + TP_FINISH_DRAWS_PER_WAVE < S ? s_first + TP_FINISH_DRAWS_PER_WAVE : S;
    const size_t e0 = (size_t)w * (size_t)S;
    const double nan = __builtin_nan(""), inf = __builtin_inf();

    double lam[SPEC_SLOTS], th[SPEC_SLOTS], oh[SPEC_SLOTS], acc[SPEC_SLOTS];
    double lo = inf, hi = -inf;
#pragma unroll
    for (int i = 0; i < SPEC_SLOTS; ++i) {
        const int j = lane + 64 * i;
        lam[i] = j < k ? a.lambda[(size_t)w * (size_t)k + j] : 0.0;
        th[i] = j < k ? a.that[(size_t)w * (size_t)k + j] : 0.0;
        oh[i] = j < k ? a.ohat[(size_t)w * (size_t)k + j] : 0.0;
        acc[i] = 0.0;
        if (j < k) { lo = pick_min(lo, lam[i]); hi = pick_max(hi, lam[i]); }
    }
    lo = wave_min(lo);                                        // (selections: the order does not matter; rounding is monotone, so
    hi = wave_max(hi);                                        //  min_j fl(lambda_j + d) = fl(min_j lambda_j + d))
    const int jst = uniform(a.jstatus[w]);
    const double n = a.n[w], kappa = a.kappa[w];
    const double c = tp_finish_greyserman_scale(a.gamma, (double)k, n);
    const double pivot_rel = (double)k * 0x1p-52;

    int first_bad = 0;
    for (int s = s_first; s < s_end; ++s) {
        const double xi = a.hyper[2 * (e0 + s)], eta = a.hyper[2 * (e0 + s) + 1];
        const double d = eta / 2;
        double* aux = a.aux + (e0 + s) * 4;
        const int st = jst != 0 ? jst : (lo + d <= pivot_rel * (hi + d) ? TP_KSTATUS_NOT_PD : 0);
        if (uniform(st) != 0) {
            if (first_bad == 0) first_bad = uniform(st);
            if (lane < 4) aux[lane] = nan;
            continue;
        }
        double uo[SPEC_SLOTS], ut[SPEC_SLOTS];
        double v[3] = {0.0, 0.0, 0.0};                        // o^'D o^, o^'D t^, t^'D t^ with D = diag(1 / (lambda_j + d))
#pragma unroll
        for (int i = 0; i < SPEC_SLOTS; ++i) {
            const double r = lane + 64 * i < k ? 1 / (lam[i] + d) : 0.0;
            uo[i] = r * oh[i];
            ut[i] = r * th[i];
            v[0] += uo[i] * oh[i];
            v[1] += uo[i] * th[i];
            v[2] += ut[i] * th[i];
        }
        wave_sums(v);
        const tp_finish_coeffs_t f = tp_finish_greyserman_coeffs(v[0], v[1], v[2], n, kappa, xi, eta, c);
#pragma unroll
        for (int i = 0; i < SPEC_SLOTS; ++i) acc[i] += f.cA * uo[i] - f.cB * ut[i];
        if (lane == 0) { aux[0] = v[0]; aux[1] = v[1]; aux[2] = v[2]; aux[3] = f.det; }
    }
    const size_t slot = (size_t)w * (size_t)NG + (size_t)g;
    double* part = a.part + slot * (size_t)k;
#pragma unroll
    for (int i = 0; i < SPEC_SLOTS; ++i) {
        const int j = lane + 64 * i;
        if (j < k) part[j] = acc[i];
    }
    if (lane == 0) a.gstatus[slot] = first_bad;
}

// One wavefront per window: w^_j = (the NG partial sums of eigen-index j in ascending order) / S, then w_i = sum_j V_ij w^_j
// with j ascending from 0 (lane l forms the rows l, l + 64, l + 128; column j of V is contiguous), the status.
__global__ __launch_bounds__(64) void spectral_window_kernel(const tp_spectral_args_t a) {
    __shared__ double what[SWEEP_MAX_K + 1];
    const int lane = threadIdx.x;
    const int S = a.S, k = a.k;
    const int NG = (S + TP_FINISH_DRAWS_PER_WAVE - 1) / TP_FINISH_DRAWS_PER_WAVE;
    const long long wl = blockIdx.x;
    const long long w = a.w_first + wl;
    const double* part = a.part + (size_t)w * (size_t)NG * (size_t)k;
    const double* V = a.V + (a.v_first + wl) * (long long)k * k;
    double* out = a.weights + (size_t)w * (size_t)k;
    int bad = 0;
    for (int g = 0; g < NG; ++g) {                            // (every lane reads the same word)
        const int gs = a.gstatus[(size_t)w * NG + g];
        if (bad == 0) bad = gs;
    }
    bad = uniform(bad);
    for (int j = lane; j < k; j += 64) {
        double sum = part[j];
        for (int g = 1; g < NG; ++g) sum += part[(size_t)g * (size_t)k + j];
        what[j] = sum / (double)S;
    }
    __syncthreads();
    bool nonfinite = false;
    for (int i = lane; i < k; i += 64) {
        double sum = 0.0;
        for (int j = 0; j < k; ++j) sum += V[(size_t)j * (size_t)k + i] * what[j];
        const double wi = bad != 0 ? __builtin_nan("") : sum;
        nonfinite = nonfinite || !finite(wi);
        out[i] = wi;
    }
    const bool any = __ballot(nonfinite) != 0;
    if (lane == 0) a.status[w] = bad != 0 ? bad : (any ? TP_KSTATUS_NONFINITE : 0);
}

}  // namespace

size_t tp_spectral_lds_bytes(int k) { return sizeof(double) * ((size_t)k * (k + 1) / 2 + 2 * (size_t)k); }

hipError_t tp_spectral_launch(const tp_spectral_args_t& a, hipStream_t st) {
    static_assert(SWEEP_MAX_K <= 64 * SPEC_SLOTS && SWEEP_MAX_K < 255, "eigen-indices per lane; a pair packs into 16 bits");
    if (a.w_count <= 0) return hipSuccess;
    const long long NG = (a.S + TP_FINISH_DRAWS_PER_WAVE - 1) / TP_FINISH_DRAWS_PER_WAVE;
    if (a.S < 1 || a.k < 1 || a.k > SWEEP_MAX_K || a.w_count * NG > 0x7fffffffLL) return hipErrorInvalidValue;
    static std::atomic<unsigned long long> attr_done{0};      // one bit per device (tp_allow_dynamic_lds)
    { hipError_t e = tp_allow_dynamic_lds(attr_done, spectral_jacobi_kernel, (int)tp_spectral_lds_bytes(SWEEP_MAX_K)); if (e != hipSuccess) return e; }
    hipLaunchKernelGGL(spectral_jacobi_kernel, dim3((unsigned)a.w_count), dim3(SWEEP_THREADS), (int)tp_spectral_lds_bytes(a.k), st, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(spectral_group_kernel, dim3((unsigned)(a.w_count * NG)), dim3(64), 0, st, a);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(spectral_window_kernel, dim3((unsigned)a.w_count), dim3(64), 0, st, a);
    return hipGetLastError();
}
