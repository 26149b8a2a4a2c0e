// posterior_size_sweep.hip - size sweep (tp_batch_size_sweep): S nested universes per window - the first k_1 < ... < k_S <= k
// columns - from ONE pair of Grams and ONE factorisation at k.
//
// The leading k_s x k_s block of S1 = a C + T (or of the Jeffreys matrix M) is the matrix the universe of size k_s
// factorises, and the L D L' factor of a leading block is the leading block of the factor.  So one workgroup per (window,
// prior) forms the packed lower triangle at k (posterior_sweep_solve.h) with one extra row per size, factorises it ONCE with
// the rows riding along, and then back-substitutes each size over its own prefix.
//
// Conjugate (a = n0 m/(m-1)), size s with k_s columns:
//     v = C[:k_s,:k_s] w0_s     q0 = a w0_s'v     c = 2 n0 / (g + sqrt(g^2 + 4 n0 q0)),  g = n0 + k_s + 2
//     w1 = S1[:k_s,:k_s]^-1 (c a v + t[:k_s])     q1 = w1'S1 w1     weights = (n1 + k_s + 2) w1 / (n1 - q1) / gamma
// One pass over the rows of C forms a C + T and, in the same pass, the S truncated products: the 32 lanes that walk row c
// keep one partial product per size - columns >= k_s are masked by the kernel, never multiplied - and meet in a fixed
// butterfly; v_s waits in row k + s of the image.  Then one wavefront per size (round-robin) forms q0_s and c_s and rewrites
// its row as c_s a v_s + t on columns < k_s, exact zeros beyond.  Entry j of a forward-substituted row depends on columns
// <= j only, so after the factorisation row k + s holds the prefix's own forward substitution on its first k_s entries:
// q1_s = sum_{j < k_s} y~_j^2 / d_j.
// Jeffreys: every size has the same right-hand side t up to truncation - ONE extra row, S back substitutions.
//
// Status per size.  Step j of the factorisation rewrites columns > j only: a bad pivot at column j leaves every prefix with
// k_s <= j intact.  The diagonal of the unfactorised matrix is kept behind the image; size s is NOT_PD when some pivot
// j < k_s has d_j <= k_s 2^-52 M_jj (the prior sweep's relative floor with the size's own k).  A NaN pivot is not "<=": it
// ends as NONFINITE, for the sizes whose prefix contains it only.
//
// The order of operations for size s depends on k_s and k only: a (window, prior, size) result does not depend on the other
// sizes, on W, P, the slot, the window's position or the sub-ranges.  Workgroup barriers only, each reached by every thread
// whatever the pivots are; none after the factorisation's last one.  Nothing spins.
#include "posterior_sweep_solve.h"
#include "posterior_size_sweep.h"

namespace {

constexpr int SIZE_WREGS = 5;                           // w0 registers per lane and size of a 32-lane row group: k <= 32 * 5
constexpr int SIZE_MAX_S = TP_SWEEP_KMAX_RHS;           // sizes per sweep
constexpr int SIZE_NWV = SWEEP_THREADS / 64;            // wavefronts of the workgroup: wave v takes sizes v, v + 4, ...
constexpr int SIZE_PER_WAVE = (SIZE_MAX_S + SIZE_NWV - 1) / SIZE_NWV;

// MAXS: the fill is unrolled over this many sizes - 4 ceil(S / 4), so that a sweep of 4 sizes does not carry the registers
// and the predicated instruction stream of 16.  The operations on a size and their order are the same in every instantiation.
template <bool CONJ, int MAXS>
__global__ void __launch_bounds__(SWEEP_THREADS) posterior_size_sweep_kernel(const tp_size_sweep_kargs_t A) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int tid = threadIdx.x;
    const int k = A.k, S = A.S;
    const int H = k + (CONJ ? S : 1);
    // priors of one window sit next to each other in the grid: the P workgroups of a window read the same C and T
    const long long wl = (long long)blockIdx.x / A.P;
    const int p = (int)((long long)blockIdx.x - wl * A.P);
    if (wl >= A.w_count) return;
    const long long w = A.w_first + wl;
    const long long wp = w * A.P + p;
    const double* __restrict__ T = A.T + wl * (long long)k * k;
    double* diag = lds + sweep_off(k, H);               // [k] diagonal of the unfactorised matrix, behind the packed image
    const int tx = tid & (SWEEP_TX - 1), ty = tid / SWEEP_TX;
    const int lane = tid & 63, wv = tid >> 6;
    double n0 = 0.0, ap = 0.0;
    double ccs[SIZE_PER_WAVE], q0s[SIZE_PER_WAVE];
#pragma unroll
    for (int r = 0; r < SIZE_PER_WAVE; ++r) { ccs[r] = 0.0; q0s[r] = 0.0; }

    if constexpr (CONJ) {
        const double* __restrict__ C = A.C + wl * (long long)k * k;
        const double* __restrict__ w0 = A.w0 + wp * (long long)S * k;
        n0 = A.n0[wp];
        const double mm = (double)(A.hf_count != nullptr ? A.hf_count[w] : A.m);
        ap = n0 * (mm / (mm - 1.0));                    // ref:333, as the run kernels form it
        // ---- load: column c of the lower triangle of a C + T from row c of the two symmetric matrices, and per size
        // v_s[c] = C[c][:k_s] w0_s[:k_s] into row k + s
        int ks[MAXS];
        double w0r[MAXS][SIZE_WREGS];
#pragma unroll
        for (int s = 0; s < MAXS; ++s) {
            ks[s] = s < S ? A.sizes[s] : 0;
#pragma unroll
            for (int q = 0; q < SIZE_WREGS; ++q) {
                const int i = tx + SWEEP_TX * q;
                w0r[s][q] = i < ks[s] ? w0[(long long)s * k + i] : 0.0;
            }
        }
        for (int c = ty; c < k; c += SWEEP_TY) {
            double* col = lds + sweep_off(c, H) - c;
            double part[MAXS];
#pragma unroll
            for (int s = 0; s < MAXS; ++s) part[s] = 0.0;
#pragma unroll
            for (int q = 0; q < SIZE_WREGS; ++q) {
                const int i = tx + SWEEP_TX * q;
                if (i < k) {
                    const double cv = C[(long long)c * k + i];
#pragma unroll
                    for (int s = 0; s < MAXS; ++s)
                        if (i < ks[s]) part[s] = fma(cv, w0r[s][q], part[s]);      // masked, not multiplied by zero
                    if (i >= c) {
                        const double sv = fma(ap, cv, T[(long long)c * k + i]);
                        col[i] = sv;
                        if (i == c) diag[c] = sv;
                    }
                }
            }
            // the 32 lanes of a row group are one half of a wavefront: these exchanges stay inside it
#pragma unroll
            for (int s = 0; s < MAXS; ++s) {
                if (s < S) {
                    double ps = part[s];
#pragma unroll
                    for (int o = SWEEP_TX / 2; o > 0; o >>= 1) ps += __shfl_xor(ps, o, 64);
                    if (tx == 0) col[k + s] = ps;
                }
            }
        }
        __syncthreads();

        // ---- per size, one wavefront: q0_s, c_s and the right-hand side c_s a v_s + t on columns < k_s, zeros beyond.
        // A lane reads and rewrites its own entries of the row only.
#pragma unroll
        for (int r = 0; r < SIZE_PER_WAVE; ++r) {
            const int s = wv + SIZE_NWV * r;
            if (s < S) {
                const int kp = A.sizes[s];
                const double* __restrict__ w0s = w0 + (long long)s * k;
                double vr[SWEEP_XREGS];
                double zp = 0.0;
#pragma unroll
                for (int q = 0; q < SWEEP_XREGS; ++q) {
                    const int i = lane + 64 * q;
                    vr[q] = 0.0;
                    if (i < kp) {
                        vr[q] = lds[sweep_off(i, H) + (k + s - i)];
                        zp = fma(w0s[i], vr[q], zp);
                    }
                }
                const double q0 = ap * wave_sum64(zp);
                const double g = n0 + kp + 2;
                const double cc = (2 * n0) / (g + sqrt(g * g + 4 * n0 * q0));      // ref:415-418
                const double ca = cc * ap;
#pragma unroll
                for (int q = 0; q < SWEEP_XREGS; ++q) {
                    const int i = lane + 64 * q;
                    if (i < k) lds[sweep_off(i, H) + (k + s - i)] = i < kp ? fma(ca, vr[q], A.t[w * k + i]) : 0.0;
                }
                ccs[r] = cc; q0s[r] = q0;
            }
        }
    } else {
        // ---- load: column c of the lower triangle = row c of the symmetric M from the diagonal on, and t as row k
        for (int c = ty; c < k; c += SWEEP_TY) {
            double* col = lds + sweep_off(c, H) - c;
            for (int i = c + tx; i < k; i += SWEEP_TX) {
                const double mv = T[(long long)c * k + i];
                col[i] = mv;
                if (i == c) diag[c] = mv;
            }
        }
        for (int c = tid; c < k; c += SWEEP_THREADS) lds[sweep_off(c, H) + (k - c)] = A.t[w * k + c];
    }
    __syncthreads();

    // ---- ONE factorisation at k with the rows riding along (posterior_sweep_solve.h).  Its single answer is not used:
    // the pivots stay on the diagonal of the image and are judged per size below.
    (void)sweep_ldl_factor(lds, k, H, tid);

    // ---- per size, one wavefront: status, q1 (ref:574), back substitution over the prefix, weights (ref:572-575, 836)
    const double n1 = n0 + (double)A.N;
    const double inv_gamma = 1.0 / A.gamma;
#pragma unroll
    for (int r = 0; r < SIZE_PER_WAVE; ++r) {
        const int s = wv + SIZE_NWV * r;
        if (s >= S) continue;
        const int kp = A.sizes[s];
        const int row = CONJ ? s : 0;
        const double rel = (double)kp * 0x1p-52;
        bool low = false;
        double qp = 0.0;
#pragma unroll
        for (int q = 0; q < SWEEP_XREGS; ++q) {
            const int j = lane + 64 * q;
            if (j < kp) {
                const double* cj = lds + sweep_off(j, H) - j;
                const double dj = cj[j];
                if (dj <= rel * diag[j]) low = true;
                qp += cj[k + row] * cj[k + row] / dj;
            }
        }
        const bool notpd = __any(low ? 1 : 0) != 0;
        const double q1 = wave_sum64(qp);
        const double denom = n1 - q1;
        double x[SWEEP_XREGS];
        sweep_back_substitute_prefix(lds, k, H, kp, row, lane, x);
        const long long e = wp * S + s;
        double* out = A.weights + e * k;
        bool bad = false;
#pragma unroll
        for (int q = 0; q < SWEEP_XREGS; ++q) {
            const int i = lane + 64 * q;
            if (i < k) {
                double v = 0.0;
                if (i < kp) {
                    if (CONJ) v = inv_gamma * ((n1 + kp + 2) * x[q] / denom);
                    else v = x[q] * inv_gamma;
                    if (!isfinite(v)) bad = true;
                }
                out[i] = v;
            }
        }
        const bool anybad = __any(bad ? 1 : 0) != 0;
        if (lane == 0) {
            int st = TP_KSTATUS_OK;
            if (notpd) st = TP_KSTATUS_NOT_PD;
            else if (anybad) st = TP_KSTATUS_NONFINITE;
            else if (CONJ && !(denom > 0.0)) st = TP_KSTATUS_BAD_DENOM;
            A.status[e] = st;
            double* ax = A.aux + e * 8;
            ax[0] = n0; ax[1] = CONJ ? n1 : 0.0; ax[2] = ccs[r]; ax[3] = q0s[r]; ax[4] = q1;
            ax[5] = CONJ ? denom : 0.0; ax[6] = 0.0; ax[7] = 0.0;
        }
    }
}

}  // namespace

// packed image at H = k + S (Jeffreys: k + 1) and the k kept diagonal elements
size_t tp_size_sweep_lds_bytes(int k, int S, bool conjugate) {
    return sizeof(double) * ((size_t)k * (k + 1) / 2 + (size_t)k * (conjugate ? S : 1) + (size_t)k);
}

hipError_t tp_size_sweep_launch(const tp_size_sweep_kargs_t& a, hipStream_t stream) {
    static_assert(SWEEP_MAX_K <= SWEEP_TX * SIZE_WREGS, "prior registers per lane");
    static_assert(SWEEP_MAX_K <= 64 * SWEEP_XREGS, "solution registers per lane");
    if (a.k < 1 || a.k > SWEEP_MAX_K || a.S < 1 || a.S > SIZE_MAX_S || a.P < 1 || a.w_count < 1) return hipErrorInvalidValue;
    const long long grid = a.w_count * (long long)a.P;
    if (grid > 0x7fffffffLL) return hipErrorInvalidValue;
    const bool conj = a.C != nullptr;
    const size_t lds = tp_size_sweep_lds_bytes(a.k, a.S, conj);
    auto go = [&](auto kernel, std::atomic<unsigned long long>& attr_done, size_t lds_max) -> hipError_t {
        const hipError_t e = tp_allow_dynamic_lds(attr_done, kernel, (int)lds_max);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(SWEEP_THREADS), lds, stream, a);
        return hipSuccess;
    };
    static std::atomic<unsigned long long> attr_done[5];      // one bit per device (tp_allow_dynamic_lds), one word per kernel
    hipError_t e;
    if (!conj) e = go(posterior_size_sweep_kernel<false, 4>, attr_done[0], tp_size_sweep_lds_bytes(SWEEP_MAX_K, 1, false));
    else if (a.S <= 4) e = go(posterior_size_sweep_kernel<true, 4>, attr_done[1], tp_size_sweep_lds_bytes(SWEEP_MAX_K, 4, true));
    else if (a.S <= 8) e = go(posterior_size_sweep_kernel<true, 8>, attr_done[2], tp_size_sweep_lds_bytes(SWEEP_MAX_K, 8, true));
    else if (a.S <= 12) e = go(posterior_size_sweep_kernel<true, 12>, attr_done[3], tp_size_sweep_lds_bytes(SWEEP_MAX_K, 12, true));
    else e = go(posterior_size_sweep_kernel<true, 16>, attr_done[4], tp_size_sweep_lds_bytes(SWEEP_MAX_K, SIZE_MAX_S, true));
    if (e != hipSuccess) return e;
    return hipGetLastError();
}
