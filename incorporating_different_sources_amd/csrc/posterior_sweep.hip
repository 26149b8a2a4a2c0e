// posterior_sweep.hip - solve sweep (tp_batch_solve_sweep): many shifts and right-hand sides per window from ONE Gram.
//
// The batch's own run kernels have stored every window's k x k matrix M_w (tp_batch_keep_posterior machinery) and its
// default right-hand side (tp_batch_keep_rhs machinery) into the sweep's workspace.  This kernel takes one workgroup per
// (window, shift): it loads M_w, adds d I + e 1 1', factorises once and solves all R right-hand sides from that one
// factorisation:
//
//     x[w][s][r] = (M_w + d_ws I + e_ws 1 1')^-1 rhs_wr / gamma
//
// Layout.  The lower triangle lives in LDS in PACKED storage, column by column, with the R right-hand sides riding along
// as R extra rows below the matrix (the border-column idea of the run kernels, turned by 90 degrees):
//
//     column c holds rows i = c .. k + R - 1 at  off(c) + (i - c),   off(c) = c (k + R) - c (c - 1) / 2
//
// k = 143 with R = 16: 12,584 doubles = 98.3 KiB of the CU's 160 KiB (full storage would not leave room for the
// right-hand sides).  A column is contiguous, so the lanes that walk down a column hit consecutive LDS banks.
//
// Factorisation: right-looking, square-root-free Cholesky M = L D L' kept UNSCALED (column j holds l_ij d_j).  Step j
// reads the pivot d_j = A[j][j] and subtracts A[i][j] A[c][j] / d_j from every element (i, c), j < c < k, c <= i < k + R.
// Nothing of column j is rewritten in step j, so ONE workgroup barrier per column is all the synchronisation there is.
// The extra rows come out as the forward substitution: row k + r ends as y~_j = (L^-1 b_r)_j = d_j (L' x_r)_j (L has a unit
// diagonal; no division by d_j has happened yet).
//
// Back substitution: one wavefront per right-hand side (wave v takes r = v, v + NW, ...), no workgroup barrier.  The
// solution stays in registers - lane l owns x_i for i = l, l + 64, l + 128 - and step j = k-1 .. 0 is a dot product of
// the contiguous column j with those registers, a wave all-reduce (fixed butterfly order) and
//     x_j = (y~_j - sum_{i > j} A[i][j] x_i) / d_j .
//
// Every (window, shift) is computed by its own workgroup from M_w, the two shift values and the R right-hand sides alone,
// in an order of operations that depends on k and R only: the result does not depend on W, S, the window's position or
// the chunking of the host loop.  Workgroup barriers only; nothing spins.
#include "posterior_sweep_solve.h"

namespace {

__global__ void __launch_bounds__(SWEEP_THREADS) posterior_sweep_kernel(const tp_sweep_kargs_t A) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int tid = threadIdx.x;
    const int k = A.k, R = A.R, H = k + R;
    // shifts of one window sit next to each other in the grid: the S workgroups of a window read the same M_w
    const long long wl = (long long)blockIdx.x / A.S;
    const int s = (int)((long long)blockIdx.x - wl * A.S);
    if (wl >= A.w_count) return;
    const long long w = A.w_first + wl;
    const double* __restrict__ M = A.post + wl * (long long)k * k;
    double sh_d = 0.0, sh_e = 0.0;
    if (A.shift != nullptr) {
        sh_d = A.shift[(w * A.S + s) * 2];
        sh_e = A.shift[(w * A.S + s) * 2 + 1];
    }
    auto off = [H](int c) { return sweep_off(c, H); };

    // ---- load: column c of the lower triangle = row c of the symmetric M_w from the diagonal on (coalesced), then the
    // R right-hand sides as rows k .. k + R - 1
    const int tx = tid & (SWEEP_TX - 1), ty = tid / SWEEP_TX;
    constexpr int TY = SWEEP_TY;
    for (int c = ty; c < k; c += TY) {
        double* col = lds + off(c) - c;
        for (int i = c + tx; i < k; i += SWEEP_TX) col[i] = M[(long long)c * k + i] + sh_e + (i == c ? sh_d : 0.0);
    }
    for (int r = 0; r < R; ++r) {
        const double* b;
        if (A.default_rhs != nullptr && r == 0) b = A.default_rhs + w * k;
        else b = A.rhs + (w * A.n_rhs + (r - (A.default_rhs != nullptr ? 1 : 0))) * (long long)k;
        for (int c = tid; c < k; c += SWEEP_THREADS) lds[off(c) + (k + r - c)] = b[c];
    }
    __syncthreads();

    // ---- factorisation with the right-hand sides riding along (posterior_sweep_solve.h)
    const bool notpd = sweep_ldl_factor(lds, k, H, tid);          // (a NaN pivot is not "<= 0": it ends as NONFINITE)

    // ---- back substitution, one wavefront per right-hand side
    const int lane = tid & 63, wv = tid >> 6;
    constexpr int NWV = SWEEP_THREADS / 64;
    const double inv_gamma = 1.0 / A.gamma;
    bool bad = false;
    for (int r = wv; r < R; r += NWV) {
        double x[SWEEP_XREGS];
        sweep_back_substitute(lds, k, H, r, lane, x);
        double* out = A.x + (((w * A.S + s) * R + r) * (long long)k);
#pragma unroll
        for (int q = 0; q < SWEEP_XREGS; ++q) {
            const int i = lane + 64 * q;
            if (i < k) {
                const double v = x[q] * inv_gamma;
                out[i] = v;
                if (!isfinite(v)) bad = true;
            }
        }
    }
    const int anybad = __syncthreads_or(bad ? 1 : 0);
    if (tid == 0) A.status[w * A.S + s] = notpd ? TP_KSTATUS_NOT_PD : anybad ? TP_KSTATUS_NONFINITE : TP_KSTATUS_OK;
}

}  // namespace

int tp_sweep_max_k(void) { return SWEEP_MAX_K; }

size_t tp_sweep_lds_bytes(int k, int R) { return sizeof(double) * ((size_t)k * (k + 1) / 2 + (size_t)k * R); }

hipError_t tp_sweep_launch(const tp_sweep_kargs_t& a, hipStream_t stream) {
    static_assert(SWEEP_MAX_K <= 64 * SWEEP_XREGS, "solution registers per lane");
    if (a.k < 1 || a.k > SWEEP_MAX_K || a.R < 1 || a.R > TP_SWEEP_KMAX_RHS || a.S < 1 || a.w_count < 1) return hipErrorInvalidValue;
    const long long grid = a.w_count * (long long)a.S;
    if (grid > 0x7fffffffLL) return hipErrorInvalidValue;
    const int lds = (int)tp_sweep_lds_bytes(a.k, a.R);
    static std::atomic<unsigned long long> attr_done{0};      // one bit per device (tp_allow_dynamic_lds)
    { hipError_t e = tp_allow_dynamic_lds(attr_done, posterior_sweep_kernel, (int)tp_sweep_lds_bytes(SWEEP_MAX_K, TP_SWEEP_KMAX_RHS)); if (e != hipSuccess) return e; }
    hipLaunchKernelGGL(posterior_sweep_kernel, dim3((unsigned)grid), dim3(SWEEP_THREADS), lds, stream, a);
    return hipGetLastError();
}
