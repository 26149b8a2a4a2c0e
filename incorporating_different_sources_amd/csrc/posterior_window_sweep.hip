// posterior_window_sweep.hip - window sweep (tp_batch_window_sweep): L nested window lengths per window - the last
// rows[w][l] daily rows - from ONE pass over the rows of the longest one.
//
// The Gram pass (posterior_window_gram_nt.hip) has stored, per window of the sub-range, the centred unscaled intraday scatter C
// (conjugate) and per length the snapshot G_l = sum x x', g_l = sum x over the length's suffix, x the batch's own rows.
//
// The correction.  The row of length l is x_r - delta_lr 1: the per-row risk-free adjustment (ref:48) depends on the mean
// calendar gap of the length's own labels.  With v = sum_r delta_r x_r, s1 = sum_r delta_r, s2 = sum_r delta_r^2 over the suffix
//
//     T = sum (x - delta 1)(x - delta 1)' = G - v 1' - 1 v' + s2 1 1'          t = sum (x - delta 1) = g - s1 1
//
// exactly.  The delta kernel forms v, s1 and s2 - one workgroup per (window, length), one thread per column, the suffix rows
// oldest first: plain VALU, about L n k flops - and runs only when the caller gave a delta.  The solve kernel applies the
// rank-two term while it forms the packed triangle; without a delta v = 0, s1 = s2 = 0 and T = G, t = g bit for bit.
//
// The solve kernel takes one workgroup per (window, prior, length) on posterior_sweep_solve.h (R = 1), like the prior sweep's:
//   conjugate  S1 = a C + T_l, v = C w0, q0, c with g = n0_wpl + k + 2, w1 = S1^-1 (c a v + t_l), n1 = n0_wpl + N_l and the
//              weights exactly as posterior_prior_sweep_kernel forms them (a = n0_wpl m/(m-1));
//   Jeffreys   M = T_l - t_l t_l'/N_l (TP_FLAG_CENTER_BY_ROWS: / rows_wl, TP_FLAG_NO_CENTER: no term), weights = M^-1 t_l / gamma,
//              aux slot 4 = t_l'M^-1 t_l.
// Pivot floor k 2^-52 of the diagonal element, statuses and aux as there.
//
// Every (window, prior, length) is computed by its own workgroup from C, its own snapshot, its delta sums, the window's
// intraday row count, the prior and N_l alone, in an order of operations that depends on k only.  Workgroup barriers only,
// each reached by every thread; nothing spins.
#include "posterior_sweep_solve.h"
#include "posterior_window_sweep.h"

namespace {

constexpr int WINDOW_WREGS = 5;         // w0 registers per lane of a 32-lane row group: k <= 32 * 5
constexpr int DELTA_THREADS = 192;      // one thread per column at k <= 143; a column loop above (the tiled window sweep)

__global__ void __launch_bounds__(DELTA_THREADS) posterior_window_delta_kernel(const tp_window_delta_kargs_t D) {
    const tp_kargs_t& A = D.in;
    const int k = A.k, L = D.L;
    const long long wl = (long long)blockIdx.x / L;
    const int l = (int)((long long)blockIdx.x - wl * L);
    if (wl >= A.w_count) return;
    const long long w = A.w_first + wl;
    const int n_w = A.n_rows ? A.n_rows[w] : A.n_r;
    const int rl = D.rows[w * L + l];
    const int* ridx = A.row_idx ? A.row_idx + w * (long long)A.n_r : nullptr;
    const long long first = A.start ? A.start[w] : 0;
    const double* sub = A.rf_adj ? A.rf_adj + w * (long long)A.n_r : nullptr;
    const double* dl = D.delta + (w * L + l) * (long long)A.n_r;
    // (no barrier below) k <= DELTA_THREADS: one column per thread; above it - the tiled window sweep - a thread takes the columns
    // j, j + DELTA_THREADS, ..., each over the same rows in the same order
    for (int j = threadIdx.x; j < k; j += DELTA_THREADS) {
        const long long col = A.col_idx ? (long long)A.col_idx[w * k + j] : (long long)j;
        double v = 0.0, s1 = 0.0, s2 = 0.0;
        for (int r = n_w - rl; r < n_w; ++r) {
            const long long row = ridx ? (long long)ridx[r] : first + r;
            double x = A.panel[row * (long long)A.panel_ld + col];
            if (sub) x -= sub[r];                            // ref:57, as the Gram pass forms the row
            const double d = dl[r];
            v = fma(d, x, v);
            s1 += d;
            s2 = fma(d, d, s2);
        }
        D.dv[(w * L + l) * (long long)k + j] = v;
        if (j == 0) {
            D.ds[(w * L + l) * 2] = s1;
            D.ds[(w * L + l) * 2 + 1] = s2;
        }
    }
}

template <bool CONJ>
__global__ void __launch_bounds__(SWEEP_THREADS) posterior_window_sweep_kernel(const tp_window_sweep_kargs_t A) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int tid = threadIdx.x;
    const int k = A.k, H = k + 1, L = A.L;
    // lengths of one (window, prior) sit next to each other in the grid, then the priors of the window: they read the same C
    const long long wp_l = (long long)blockIdx.x / L;
    const int l = (int)((long long)blockIdx.x - wp_l * L);
    const long long wl = wp_l / A.P;
    const int p = (int)(wp_l - wl * A.P);
    if (wl >= A.w_count) return;
    const long long w = A.w_first + wl;
    const long long wp = w * A.P + p;
    const long long e = wp * L + l;
    const long long wlen = w * L + l;
    const double* __restrict__ T = A.T + (wl * L + l) * (long long)k * k;
    double* vbuf = lds + sweep_off(k, H);                // [k] v = C w0, behind the packed image
    double* floor = vbuf + k;                            // [k] pivot floors: k 2^-52 times the diagonal element
    double* tbuf = floor + k;                            // [k] t_l = g_l - s1
    double* dvb = tbuf + k;                              // [k] the delta kernel's v (zeros without a delta)
    const double rel = (double)k * 0x1p-52;
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
    double n0 = 0.0, cc = 0.0, q0 = 0.0;
    if constexpr (CONJ) {
        const double* __restrict__ C = A.C + wl * (long long)k * k;
        const double* __restrict__ w0 = A.w0 + wp * k;
        n0 = A.n0[e];
        const double mm = (double)(A.hf_count != nullptr ? A.hf_count[w] : A.m);
        const double ap = n0 * (mm / (mm - 1.0));            // ref:333, as the run kernels form it
        // ---- load: column c of the lower triangle of S1 = a C + T_l from row c of the symmetric matrices, v_c = C[c][:] w0
        double w0r[WINDOW_WREGS];
#pragma unroll
        for (int q = 0; q < WINDOW_WREGS; ++q) {
            const int i = tx + SWEEP_TX * q;
            w0r[q] = i < k ? w0[i] : 0.0;
        }
        for (int c = ty; c < k; c += SWEEP_TY) {
            double* col = lds + sweep_off(c, H) - c;
            const double dc = dvb[c];
            double part = 0.0;
#pragma unroll
            for (int q = 0; q < WINDOW_WREGS; ++q) {
                const int i = tx + SWEEP_TX * q;
                if (i < k) {
                    const double cv = C[(long long)c * k + i];
                    part = fma(cv, w0r[q], part);
                    if (i >= c) {
                        const double tv = T[(long long)c * k + i] - dc - dvb[i] + s2;     // G - v 1' - 1 v' + s2 1 1'
                        const double sv = fma(ap, cv, tv);
                        col[i] = sv;
                        if (i == c) floor[c] = rel * sv;
                    }
                }
            }
            // the 32 lanes of a row group are one half of a wavefront: these exchanges stay inside it
#pragma unroll
            for (int o = SWEEP_TX / 2; o > 0; o >>= 1) part += __shfl_xor(part, o, 64);
            if (tx == 0) vbuf[c] = part;
        }
        __syncthreads();

        // ---- q0, c and the right-hand side c a v + t_l as row k (every wavefront forms the same q0 in the same order)
        double zp = 0.0;
#pragma unroll
        for (int q = 0; q < SWEEP_XREGS; ++q) {
            const int i = lane + 64 * q;
            if (i < k) zp = fma(w0[i], vbuf[i], zp);
        }
        q0 = ap * wave_sum64(zp);
        const double g = n0 + k + 2;
        cc = (2 * n0) / (g + sqrt(g * g + 4 * n0 * q0));       // ref:415-418
        const double ca = cc * ap;
        for (int c = tid; c < k; c += SWEEP_THREADS) lds[sweep_off(c, H) + (k - c)] = fma(ca, vbuf[c], tbuf[c]);
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
                if (i == c) floor[c] = rel * mv;
            }
        }
        for (int c = tid; c < k; c += SWEEP_THREADS) lds[sweep_off(c, H) + (k - c)] = tbuf[c];
    }
    __syncthreads();

    // ---- factorisation with the right-hand side riding along (posterior_sweep_solve.h).  A pivot that is no more than
    // k 2^-52 of its diagonal element is rounding noise: the matrix is singular to working precision.  (A NaN pivot is not
    // "<=": it ends as NONFINITE)
    const bool notpd = sweep_ldl_factor(lds, k, H, tid, floor);

    // ---- wave 0: q1 = sum y~_j^2 / d_j (ref:574), back substitution, weights (ref:572-575, 836; Jeffreys: ref:606, 849)
    bool bad = false;
    double q1 = 0.0, denom = 0.0;
    const double n1 = n0 + Nl;
    if (wv == 0) {
        double qp = 0.0;
#pragma unroll
        for (int q = 0; q < SWEEP_XREGS; ++q) {
            const int j = lane + 64 * q;
            if (j < k) {
                const double* cj = lds + sweep_off(j, H) - j;
                qp += cj[k] * cj[k] / cj[j];
            }
        }
        q1 = wave_sum64(qp);
        denom = n1 - q1;
        double x[SWEEP_XREGS];
        sweep_back_substitute(lds, k, H, 0, lane, x);
        double* out = A.weights + e * k;
#pragma unroll
        for (int q = 0; q < SWEEP_XREGS; ++q) {
            const int i = lane + 64 * q;
            if (i < k) {
                const double v = CONJ ? 1.0 / A.gamma * ((n1 + k + 2) * x[q] / denom) : x[q] * (1.0 / A.gamma);
                out[i] = v;
                if (!isfinite(v)) bad = true;
            }
        }
    }
    const int anybad = __syncthreads_or(bad ? 1 : 0);
    if (tid == 0) {
        int st = TP_KSTATUS_OK;
        if (notpd) st = TP_KSTATUS_NOT_PD;
        else if (anybad) st = TP_KSTATUS_NONFINITE;
        else if (CONJ && !(denom > 0.0)) st = TP_KSTATUS_BAD_DENOM;
        A.status[e] = st;
        double* ax = A.aux + e * 8;
        ax[0] = n0; ax[1] = CONJ ? n1 : 0.0; ax[2] = cc; ax[3] = q0; ax[4] = q1; ax[5] = CONJ ? denom : 0.0; ax[6] = 0.0; ax[7] = 0.0;
    }
}

}  // namespace

// packed image at H = k + 1, then v, the pivot floors, t_l and the delta kernel's v
size_t tp_window_sweep_lds_bytes(int k) { return sizeof(double) * ((size_t)k * (k + 3) / 2 + 4 * (size_t)k); }

hipError_t tp_window_sweep_launch(const tp_window_sweep_kargs_t& a, hipStream_t stream) {
    static_assert(SWEEP_MAX_K <= SWEEP_TX * WINDOW_WREGS, "prior registers per lane");
    static_assert(SWEEP_MAX_K <= 64 * SWEEP_XREGS, "solution registers per lane");
    if (a.k < 1 || a.k > SWEEP_MAX_K || a.P < 1 || a.L < 1 || a.L > TP_SWEEP_KMAX_RHS || a.w_count < 1) return hipErrorInvalidValue;
    const long long grid = a.w_count * (long long)a.P * a.L;
    if (grid > 0x7fffffffLL) return hipErrorInvalidValue;
    static std::atomic<unsigned long long> attr_done[2];      // one bit per device (tp_allow_dynamic_lds), one word per kernel
    const int lds_max = (int)tp_window_sweep_lds_bytes(SWEEP_MAX_K);
    if (a.C != nullptr) {
        const hipError_t e = tp_allow_dynamic_lds(attr_done[0], posterior_window_sweep_kernel<true>, lds_max);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(posterior_window_sweep_kernel<true>, dim3((unsigned)grid), dim3(SWEEP_THREADS), tp_window_sweep_lds_bytes(a.k), stream, a);
    } else {
        const hipError_t e = tp_allow_dynamic_lds(attr_done[1], posterior_window_sweep_kernel<false>, lds_max);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(posterior_window_sweep_kernel<false>, dim3((unsigned)grid), dim3(SWEEP_THREADS), tp_window_sweep_lds_bytes(a.k), stream, a);
    }
    return hipGetLastError();
}

hipError_t tp_window_delta_launch(const tp_window_delta_kargs_t& a, hipStream_t stream) {
    if (a.in.k < 1 || a.L < 1 || a.in.w_count < 1) return hipErrorInvalidValue;
    const long long grid = a.in.w_count * (long long)a.L;
    if (grid > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(posterior_window_delta_kernel, dim3((unsigned)grid), dim3(DELTA_THREADS), 0, stream, a);
    return hipGetLastError();
}

// Gram pass: dispatcher over the tile count NT = ceil((k+1)/16) (posterior_window_gram_nt.hip, one translation unit per tile count)
#define TP_DECL(NT) hipError_t tp_window_gram_launch_nt##NT(const tp_window_gram_kargs_t&, hipStream_t);
TP_DECL(1) TP_DECL(2) TP_DECL(3) TP_DECL(4) TP_DECL(5) TP_DECL(6) TP_DECL(7) TP_DECL(8) TP_DECL(9)
#undef TP_DECL

hipError_t tp_window_gram_launch(const tp_window_gram_kargs_t& g, hipStream_t stream) {
    if (g.in.k < 1 || g.in.k > SWEEP_MAX_K || g.L < 1 || g.in.w_count < 1 || g.in.w_count > 0x7ffffff0LL) return hipErrorInvalidValue;
    switch ((g.in.k + 1 + 15) / 16) {
#define TP_CASE(NT) case NT: return tp_window_gram_launch_nt##NT(g, stream);
        TP_CASE(1) TP_CASE(2) TP_CASE(3) TP_CASE(4) TP_CASE(5) TP_CASE(6) TP_CASE(7) TP_CASE(8) TP_CASE(9)
#undef TP_CASE
        default: return hipErrorInvalidValue;
    }
}
