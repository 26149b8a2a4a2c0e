// posterior_grid_sweep.hip - grid sweep (tp_batch_grid_sweep): S nested universes x L nested window lengths per window from
// ONE segmented Gram pass and ONE factorisation per (window, prior, length).
//
// The two nestings are independent.  The window sweep's snapshot (T_l, t_l) of length l, taken at the largest size k, holds
// the snapshot of every smaller universe as its leading block - a Gram entry (i, j) is a sum over rows of x_i x_j and knows
// nothing of the other columns -, and so do C, the delta sums v and the rank-two correction.  The size sweep's argument then
// applies to every length: the leading k_s x k_s block of a C + T_l (or of the Jeffreys matrix M_l) is the matrix the universe
// of size k_s factorises over length l, and the L D L' factor of a leading block is the leading block of the factor.  So one
// workgroup per (window, prior, length) loads the matrix as posterior_window_sweep_kernel does - the correction
// T = G - v 1' - 1 v' + s2 1 1', t = g - s1 1 evaluated from left to right - and goes on as posterior_size_sweep_kernel does:
// one extra row per size, ONE factorisation at k with the rows riding along, one prefix back substitution per size.
//
// Conjugate (a = n0_wpl m/(m-1)), size s with k_s columns:
//     v = C[:k_s,:k_s] w0_s     q0 = a w0_s'v     c = 2 n0 / (g + sqrt(g^2 + 4 n0 q0)),  g = n0_wpl + k_s + 2
//     w1 = S1[:k_s,:k_s]^-1 (c a v + t_l[:k_s])     q1 = w1'S1 w1     weights = (n1 + k_s + 2) w1 / (n1 - q1) / gamma,  n1 = n0_wpl + N_l
// One pass over the rows of C forms the triangle and the S truncated products - columns >= k_s masked, never multiplied -,
// reduced in a fixed butterfly and parked in row k + s of the image; one wavefront per size (round-robin) forms q0_s and c_s
// and rewrites its row as c_s a v_s + t_l on columns < k_s, exact zeros beyond.
// Jeffreys: M = T_l - t_l t_l'/N_l (TP_FLAG_CENTER_BY_ROWS: / rows_wl, TP_FLAG_NO_CENTER: no term) formed here from the snapshot,
// t_l as the ONE extra row, S back substitutions.
//
// Status per size from the kept diagonal of the unfactorised matrix: NOT_PD when some pivot j < k_s has d_j <= k_s 2^-52 M_jj;
// a NaN pivot is not "<=" and ends as NONFINITE, for the sizes whose prefix contains it only.
//
// The order of operations for (length l, size s) depends on k_s and k only: an entry does not depend on the other sizes, on
// W, P, the slot, the window's position or the sub-ranges.  Workgroup barriers only, each reached by every thread whatever the
// pivots are; none after the factorisation's last one.  Nothing spins.
#include "posterior_sweep_solve.h"
#include "posterior_grid_sweep.h"

namespace {

constexpr int GRID_WREGS = 5;                           // w0 registers per lane and size of a 32-lane row group: k <= 32 * 5
constexpr int GRID_MAX_S = TP_SWEEP_KMAX_RHS;           // sizes per sweep
constexpr int GRID_NWV = SWEEP_THREADS / 64;            // wavefronts of the workgroup: wave v takes sizes v, v + 4, ...
constexpr int GRID_PER_WAVE = (GRID_MAX_S + GRID_NWV - 1) / GRID_NWV;

// MAXS: the fill is unrolled over this many sizes - 4 ceil(S / 4), as the size sweep's is.  The operations on a size and their
// order are the same in every instantiation.
// Two wavefronts per SIMD are asked for: without the bound the 16-size build took 264 registers - one workgroup per CU where
// the LDS image (55.6 KB at k = 100, S = 16) lets two run - and a sweep of 16 sizes 1.6 - 1.8x the device time;
// with it 231, no scratch.
template <bool CONJ, int MAXS>
__global__ void __launch_bounds__(SWEEP_THREADS, 2) posterior_grid_sweep_kernel(const tp_grid_sweep_kargs_t A) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int tid = threadIdx.x;
    const int k = A.k, S = A.S, L = A.L;
    const int H = k + (CONJ ? S : 1);
    // lengths of one (window, prior) sit next to each other in the grid, then the priors of the window: they read the same C
    const long long wp_l = (long long)blockIdx.x / L;
    const int l = (int)((long long)blockIdx.x - wp_l * L);
    const long long wl = wp_l / A.P;
    const int p = (int)(wp_l - wl * A.P);
    if (wl >= A.w_count) return;
    const long long w = A.w_first + wl;
    const long long wp = w * A.P + p;
    const long long wpl = wp * L + l;
    const long long wlen = w * L + l;
    const double* __restrict__ T = A.T + (wl * L + l) * (long long)k * k;
    double* diag = lds + sweep_off(k, H);               // [k] diagonal of the unfactorised matrix, behind the packed image
    double* tbuf = diag + k;                            // [k] t_l = g_l - s1
    double* dvb = tbuf + k;                             // [k] the delta kernel's v (zeros without a delta)
    const double s1 = A.ds != nullptr ? A.ds[wlen * 2] : 0.0;
    const double s2 = A.ds != nullptr ? A.ds[wlen * 2 + 1] : 0.0;
    const double Nl = (double)A.N[l];

    for (int c = tid; c < k; c += SWEEP_THREADS) {
        tbuf[c] = A.t[wlen * k + c] - s1;
        dvb[c] = A.dv != nullptr ? A.dv[wlen * k + c] : 0.0;
    }
    __syncthreads();

    const int tx = tid & (SWEEP_TX - 1), ty = tid / SWEEP_TX;
    const int lane = tid & 63, wv = tid >> 6;
    double n0 = 0.0, ap = 0.0;
    double ccs[GRID_PER_WAVE], q0s[GRID_PER_WAVE];
#pragma unroll
    for (int r = 0; r < GRID_PER_WAVE; ++r) { ccs[r] = 0.0; q0s[r] = 0.0; }

    if constexpr (CONJ) {
        const double* __restrict__ C = A.C + wl * (long long)k * k;
        const double* __restrict__ w0 = A.w0 + wp * (long long)S * k;
        n0 = A.n0[wpl];
        const double mm = (double)(A.hf_count != nullptr ? A.hf_count[w] : A.m);
        ap = n0 * (mm / (mm - 1.0));                    // ref:333, as the run kernels form it
        // ---- load: column c of the lower triangle of S1 = a C + T_l from row c of the symmetric matrices, and per size
        // v_s[c] = C[c][:k_s] w0_s[:k_s] into row k + s
        int ks[MAXS];
        double w0r[MAXS][GRID_WREGS];
#pragma unroll
        for (int s = 0; s < MAXS; ++s) {
            ks[s] = s < S ? A.sizes[s] : 0;
#pragma unroll
            for (int q = 0; q < GRID_WREGS; ++q) {
                const int i = tx + SWEEP_TX * q;
                w0r[s][q] = i < ks[s] ? w0[(long long)s * k + i] : 0.0;
            }
        }
        for (int c = ty; c < k; c += SWEEP_TY) {
            double* col = lds + sweep_off(c, H) - c;
            const double dc = dvb[c];
            double part[MAXS];
#pragma unroll
            for (int s = 0; s < MAXS; ++s) part[s] = 0.0;
#pragma unroll
            for (int q = 0; q < GRID_WREGS; ++q) {
                const int i = tx + SWEEP_TX * q;
                if (i < k) {
                    const double cv = C[(long long)c * k + i];
#pragma unroll
                    for (int s = 0; s < MAXS; ++s)
                        if (i < ks[s]) part[s] = fma(cv, w0r[s][q], part[s]);      // masked, not multiplied by zero
                    if (i >= c) {
                        const double tv = T[(long long)c * k + i] - dc - dvb[i] + s2;     // G - v 1' - 1 v' + s2 1 1'
                        const double sv = fma(ap, cv, tv);
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

        // ---- per size, one wavefront: q0_s, c_s and the right-hand side c_s a v_s + t_l on columns < k_s, zeros beyond.
        // A lane reads and rewrites its own entries of the row only.
#pragma unroll
        for (int r = 0; r < GRID_PER_WAVE; ++r) {
            const int s = wv + GRID_NWV * r;
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
                    if (i < k) lds[sweep_off(i, H) + (k + s - i)] = i < kp ? fma(ca, vr[q], tbuf[i]) : 0.0;
                }
                ccs[r] = cc; q0s[r] = q0;
            }
        }
    } else {
        // ---- load: column c of the lower triangle of M = T_l - t_l t_l'/N_l (ref:600) or its flagged form, t_l as row k
        const double div = A.center_rows == 1 ? (double)A.rows[wlen] : Nl;
        const double rinv = A.center_rows == 2 ? 0.0 : 1.0 / div;
        for (int c = ty; c < k; c += SWEEP_TY) {
            double* col = lds + sweep_off(c, H) - c;
            const double dc = dvb[c];
            const double tc = -(tbuf[c] * rinv);
            for (int i = c + tx; i < k; i += SWEEP_TX) {
                const double tv = T[(long long)c * k + i] - dc - dvb[i] + s2;
                const double mv = A.center_rows == 2 ? tv : fma(tc, tbuf[i], tv);
                col[i] = mv;
                if (i == c) diag[c] = mv;
            }
        }
        for (int c = tid; c < k; c += SWEEP_THREADS) lds[sweep_off(c, H) + (k - c)] = tbuf[c];
    }
    __syncthreads();

    // ---- ONE factorisation at k with the rows riding along (posterior_sweep_solve.h).  Its single answer is not used:
    // the pivots stay on the diagonal of the image and are judged per size below.
    (void)sweep_ldl_factor(lds, k, H, tid);

    // ---- per size, one wavefront: status, q1 (ref:574), back substitution over the prefix, weights (ref:572-575, 836;
    // Jeffreys: ref:606, 849)
    const double n1 = n0 + Nl;
    const double inv_gamma = 1.0 / A.gamma;
#pragma unroll
    for (int r = 0; r < GRID_PER_WAVE; ++r) {
        const int s = wv + GRID_NWV * r;
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
        const long long e = wpl * S + s;
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

// packed image at H = k + S (Jeffreys: k + 1), the k kept diagonal elements, t_l - s1 and the delta kernel's v
size_t tp_grid_sweep_lds_bytes(int k, int S, bool conjugate) {
    return sizeof(double) * ((size_t)k * (k + 1) / 2 + (size_t)k * (conjugate ? S : 1) + 3 * (size_t)k);
}

hipError_t tp_grid_sweep_launch(const tp_grid_sweep_kargs_t& a, hipStream_t stream) {
    static_assert(SWEEP_MAX_K <= SWEEP_TX * GRID_WREGS, "prior registers per lane");
    static_assert(SWEEP_MAX_K <= 64 * SWEEP_XREGS, "solution registers per lane");
    if (a.k < 1 || a.k > SWEEP_MAX_K || a.S < 1 || a.S > GRID_MAX_S || a.L < 1 || a.L > TP_SWEEP_KMAX_RHS || a.P < 1 || a.w_count < 1)
        return hipErrorInvalidValue;
    const long long grid = a.w_count * (long long)a.P * a.L;
    if (grid > 0x7fffffffLL) return hipErrorInvalidValue;
    const bool conj = a.C != nullptr;
    const size_t lds = tp_grid_sweep_lds_bytes(a.k, a.S, conj);
    auto go = [&](auto kernel, std::atomic<unsigned long long>& attr_done, size_t lds_max) -> hipError_t {
        const hipError_t e = tp_allow_dynamic_lds(attr_done, kernel, (int)lds_max);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(SWEEP_THREADS), lds, stream, a);
        return hipSuccess;
    };
    static std::atomic<unsigned long long> attr_done[5];      // one bit per device (tp_allow_dynamic_lds), one word per kernel
    hipError_t e;
    if (!conj) e = go(posterior_grid_sweep_kernel<false, 4>, attr_done[0], tp_grid_sweep_lds_bytes(SWEEP_MAX_K, 1, false));
    else if (a.S <= 4) e = go(posterior_grid_sweep_kernel<true, 4>, attr_done[1], tp_grid_sweep_lds_bytes(SWEEP_MAX_K, 4, true));
    else if (a.S <= 8) e = go(posterior_grid_sweep_kernel<true, 8>, attr_done[2], tp_grid_sweep_lds_bytes(SWEEP_MAX_K, 8, true));
    else if (a.S <= 12) e = go(posterior_grid_sweep_kernel<true, 12>, attr_done[3], tp_grid_sweep_lds_bytes(SWEEP_MAX_K, 12, true));
    else e = go(posterior_grid_sweep_kernel<true, 16>, attr_done[4], tp_grid_sweep_lds_bytes(SWEEP_MAX_K, GRID_MAX_S, true));
    if (e != hipSuccess) return e;
    return hipGetLastError();
}
