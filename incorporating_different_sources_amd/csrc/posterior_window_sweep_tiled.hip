// posterior_window_sweep_tiled.hip - window sweep above the LDS solve core (tp_batch_window_sweep_tiled, k > tp_sweep_max_assets()):
// L nested window lengths per window from ONE pass over the rows of the longest one, factorised by the large-k tiled pipeline.
//
// Per window of the sub-range the Gram stage has stored: conjugate, C = Y'Y - (Y'1)(Y'1)'/m (k x k, symmetric, full storage:
// the batch's own tiled Gram stage over the intraday rows, steered by its arguments as for tp_batch_prior_sweep_tiled); per
// length the snapshot G_l = sum x x' (column >= row) and g_l = sum x over the length's suffix (the segmented Gram,
// posterior_tiled_window_wave.h); with a delta, the sums v, s1, s2 of the rank-two correction (posterior_window_sweep.hip).
// An ARENA ENTRY is one (window, prior, length); the entries of one launch share the length, so that tp_tiled_factor_launch
// factorises and solves them with N = N[l] as it does the windows of a run.  The kernels here leave in the arena, in ws.scal and
// in ws.flags what tiled_clear_kernel leaves for a run:
//
//   window_sweep_tiled_cw_kernel      one workgroup per (window, prior): u = C w0 and w0'u, once - they depend on neither the
//                                     length nor n0
//   window_sweep_tiled_fill_kernel    one workgroup per (entry, super-tile (I, J), I <= J).  With T = G_l - v 1' - 1 v' + s2 1 1'
//                                     evaluated left to right as the LDS sweep does (v = 0, s1 = s2 = 0: the bits of G_l) and
//                                     t = g_l - s1 1:  conjugate a C + T with a = n0_wpl m/(m-1), column k = c a u + t, q0 = a w0'u
//                                     and c as in ref:415-418 with g = n0_wpl + k + 2;  Jeffreys T - t t'/N_l (TP_FLAG_CENTER_BY_ROWS:
//                                     / rows_wl, TP_FLAG_NO_CENTER: no term), column k = t
//   window_sweep_tiled_border_kernel  one workgroup per entry: ws.scal = (s, sqrt s, c, q0, n0), rows >= k and the flag zeroed
//                                     (close_entry)
//   window_sweep_tiled_scatter_kernel one workgroup per entry, behind the factorisation: weights, status and aux from the
//                                     launch's staging rows to slot (w P + p) L + l of the sweep's results
//
// The grid decode, the conjugate scalars and the closing of an entry are posterior_tiled_sweep_prims.h's.
//
// C is RAW-MOMENT centred as in the tiled prior sweep.  Plain C++, workgroup barriers only, each reached
// by every thread of its workgroup; every loop is bounded by k, KP or the launch's arguments.  A (window, prior, length) result
// depends on the window's C, its own snapshot and delta sums, its prior, N_l and k alone: every sum runs in an order fixed by k.
#include "posterior_tiled_sweep_prims.h"
#include "posterior_window_sweep.h"

namespace {

constexpr int CW_MAX_K = 2048;

__global__ void __launch_bounds__(NTHREADS) window_sweep_tiled_cw_kernel(const tp_window_sweep_tiled_kargs_t A) {
    __shared__ double u[CW_MAX_K];
    __shared__ double red[4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int k = A.k;
    const long long wp = A.wp_first + blockIdx.x;
    const long long w = wp / A.P;
    const long long wpl = wp - A.wc_first * A.P;               // the pair's number inside the sub-range
    const double* __restrict__ C = A.C + (w - A.wc_first) * (long long)k * k;
    const double* __restrict__ w0 = A.w0 + wp * k;
    // a wavefront per row of the symmetric C: lane l takes the columns l, l + 64, ...
    for (int i = wv; i < k; i += NTHREADS / 64) {
        const double* __restrict__ row = C + (long long)i * k;
        double s = 0.0;
        for (int c = lane; c < k; c += 64) s = fma(row[c], w0[c], s);
        s = wave_sum64(s);
        if (lane == 0) u[i] = s;
    }
    __syncthreads();
    double q = 0.0;
    for (int i = tid; i < k; i += NTHREADS) {
        const double v = u[i];
        A.cw[wpl * k + i] = v;
        q = fma(w0[i], v, q);
    }
    q = wave_sum64(q);
    if (lane == 0) red[wv] = q;
    __syncthreads();
    if (tid == 0) A.cq[wpl] = sum4(red);
}

// the scalars of entry `wp`, length A.l (conjugate): every workgroup of the entry forms them from the same numbers in the same way
__device__ __forceinline__ EntryScal entry_scalars(const tp_window_sweep_tiled_kargs_t& A, const long long wp, const long long w) {
    EntryScal sc;
    sc.n0 = A.n0[wp * A.L + A.l];
    sc.s = prior_scale(sc.n0, hf_rows(A, w));
    sc.q0 = sc.s * A.cq[wp - A.wc_first * A.P];
    sc.c = shrink_c(sc.n0, A.k, sc.q0);
    return sc;
}

template <bool CONJ>
__global__ void __launch_bounds__(NTHREADS) window_sweep_tiled_fill_kernel(const tp_window_sweep_tiled_kargs_t A, const tp_tiled_ws_t ws) {
    __shared__ double tI[SB], tJ[SB], dI[SB], dJ[SB];          // t = g_l - s1 and the delta kernel's v of the tile's rows / columns
    const int tid = threadIdx.x;
    const int k = A.k, KP = ws.KP, NS = ws.NS, L = A.L;
    long long e;
    int I, J;
    if (!xcd_entry_tile(NS, A.e_count, e, I, J)) return;
    const long long wp = A.wp_first + e;
    const long long w = wp / A.P;
    const long long wl = w - A.wc_first;
    const long long wlen = w * L + A.l;
    const double* __restrict__ T = A.T + (wl * L + A.l) * (long long)k * k;
    const double* __restrict__ tg = A.t + wlen * k;
    const double s1 = A.ds != nullptr ? A.ds[wlen * 2] : 0.0;
    const double s2 = A.ds != nullptr ? A.ds[wlen * 2 + 1] : 0.0;
    double* M = ws.arena + e * (long long)KP * KP;

    if (tid < 2 * SB) {
        const int x = tid & (SB - 1);
        const int g = SB * (tid < SB ? I : J) + x;
        const double tv = g < k ? tg[g] - s1 : 0.0;
        const double dv = (g < k && A.dv != nullptr) ? A.dv[wlen * k + g] : 0.0;
        if (tid < SB) { tI[x] = tv; dI[x] = dv; } else { tJ[x] = tv; dJ[x] = dv; }
    }
    __syncthreads();
    EntryScal es{0.0, 0.0, 0.0, 0.0};
    const double* __restrict__ C = nullptr;
    const double* __restrict__ cw = nullptr;
    double rinv = 0.0;
    if constexpr (CONJ) {
        es = entry_scalars(A, wp, w);
        C = A.C + wl * (long long)k * k;
        cw = A.cw + (wp - A.wc_first * A.P) * k;
    } else {
        rinv = A.center_rows == 2 ? 0.0 : 1.0 / (A.center_rows == 1 ? (double)A.rows[wlen] : (double)A.N);
    }
    const int c = tid & (SB - 1), q = tid >> 6;
    const int gj = SB * J + c;
    for (int r = q; r < SB; r += NTHREADS / SB) {
        const int gi = SB * I + r;
        double out = 0.0;
        if (gi < k && gj < k) {
            // element (lo, hi) of the upper triangle; a diagonal super-tile mirrors it below its diagonal
            const bool up = I < J || r <= c;
            const int lo = up ? gi : gj, hi = up ? gj : gi;
            const double dlo = up ? dI[r] : dJ[c], dhi = up ? dJ[c] : dI[r];
            const double tv = T[(long long)lo * k + hi] - dlo - dhi + s2;      // G - v 1' - 1 v' + s2 1 1'
            if constexpr (CONJ) {
                out = fma(es.s, C[(long long)gi * k + gj], tv);
            } else {
                const double tlo = up ? tI[r] : tJ[c], thi = up ? tJ[c] : tI[r];
                out = A.center_rows == 2 ? tv : fma(-(tlo * rinv), thi, tv);
            }
        } else if (gj == k && gi < k) {
            out = CONJ ? fma(es.c * es.s, cw[gi], tI[r]) : tI[r];
        }
        M[(long long)gi * KP + gj] = out;
    }
}

template <bool CONJ>
__global__ void __launch_bounds__(NTHREADS) window_sweep_tiled_border_kernel(const tp_window_sweep_tiled_kargs_t A, const tp_tiled_ws_t ws) {
    const long long e = blockIdx.x;
    EntryScal es{0.0, 0.0, 0.0, 0.0};
    if constexpr (CONJ) es = entry_scalars(A, A.wp_first + e, (A.wp_first + e) / A.P);
    close_entry(ws, e, A.k, es);
}

__global__ void __launch_bounds__(NTHREADS) window_sweep_tiled_scatter_kernel(const tp_window_sweep_tiled_kargs_t A) {
    const int tid = threadIdx.x;
    const long long e = blockIdx.x;
    const int k = A.k;
    const long long f = (A.wp_first + e) * A.L + A.l;
    for (int i = tid; i < k; i += NTHREADS) A.weights[f * k + i] = A.stage_w[e * k + i];
    if (tid < 8) A.aux[f * 8 + tid] = A.stage_a[e * 8 + tid];
    if (tid == 0) A.status[f] = A.stage_s[e];
}

bool args_ok(const tp_window_sweep_tiled_kargs_t& a) {
    return a.k >= 1 && a.k < CW_MAX_K && a.P >= 1 && a.L >= 1 && a.l >= 0 && a.l < a.L && a.e_count >= 1 && a.e_count <= 65535;
}

}  // namespace

hipError_t tp_window_sweep_tiled_cw_launch(const tp_window_sweep_tiled_kargs_t& a, hipStream_t stream) {
    // (e_count: the (window, prior) pairs of a whole sub-range here, not the entries of one arena group)
    if (a.k < 1 || a.k >= CW_MAX_K || a.P < 1 || a.e_count < 1 || a.e_count > 0x7fffffffLL || a.C == nullptr || a.cw == nullptr || a.cq == nullptr)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(window_sweep_tiled_cw_kernel, dim3((unsigned)a.e_count), dim3(NTHREADS), 0, stream, a);
    return hipGetLastError();
}

hipError_t tp_window_sweep_tiled_fill_launch(const tp_window_sweep_tiled_kargs_t& a, const tp_tiled_ws_t& ws, hipStream_t stream) {
    if (!args_ok(a)) return hipErrorInvalidValue;
    const dim3 grid = xcd_entry_grid(ws.NS, a.e_count);
    if (a.C != nullptr) {
        hipLaunchKernelGGL(window_sweep_tiled_fill_kernel<true>, grid, dim3(NTHREADS), 0, stream, a, ws);
        hipLaunchKernelGGL(window_sweep_tiled_border_kernel<true>, dim3((unsigned)a.e_count), dim3(NTHREADS), 0, stream, a, ws);
    } else {
        hipLaunchKernelGGL(window_sweep_tiled_fill_kernel<false>, grid, dim3(NTHREADS), 0, stream, a, ws);
        hipLaunchKernelGGL(window_sweep_tiled_border_kernel<false>, dim3((unsigned)a.e_count), dim3(NTHREADS), 0, stream, a, ws);
    }
    return hipGetLastError();
}

hipError_t tp_window_sweep_tiled_scatter_launch(const tp_window_sweep_tiled_kargs_t& a, hipStream_t stream) {
    if (!args_ok(a)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(window_sweep_tiled_scatter_kernel, dim3((unsigned)a.e_count), dim3(NTHREADS), 0, stream, a);
    return hipGetLastError();
}
