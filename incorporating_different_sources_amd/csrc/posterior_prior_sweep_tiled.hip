// posterior_prior_sweep_tiled.hip - prior sweep above the LDS solve core (tp_batch_prior_sweep_tiled, k > tp_sweep_max_assets()):
// many conjugate priors (n0, w0) per window from ONE pair of Grams, factorised by the large-k tiled pipeline.
//
// The Gram stage of the tiled path (tp_tiled_gram_launch, steered by its arguments: tangency_api.cpp) has stored, per window of
// the sub-range, T = X'X and C = Y'Y - (Y'1)(Y'1)'/m (both k x k, symmetric, full storage) and t = X'1.  An ARENA ENTRY is one
// (window, prior) pair; with a = n0 m/(m-1) the two kernels here leave in the arena, in ws.scal and in ws.flags exactly what
// tiled_clear_kernel leaves for a conjugate run, so that tp_tiled_factor_launch factorises and solves the entries as it does
// windows:
//
//   prior_sweep_tiled_fill_kernel     one workgroup per (entry, super-tile (I, J), I <= J): a C + T into the arena tile, t into
//                                     column k, and the 64-row pieces of a C w0 the tile contributes (rows of I from the
//                                     columns of J and, I < J, rows of J from the columns of I: C is symmetric)
//   prior_sweep_tiled_border_kernel   one workgroup per entry: the border of a conjugate entry (conj_border, close_entry) -
//                                     the arithmetic of tiled_clear_kernel's shared-intraday branch, by the same functions
//
// The grid decode, the conjugate scalars, the tile products and the border are posterior_tiled_sweep_prims.h's.
//
// C is RAW-MOMENT centred (the Gram kernels' row-count centring, center_rows = 1), not shifted by a row of the window like the
// run kernels' S0: exact to rounding while the intraday mean is small against the spread (returns), it loses digits under a
// large common offset of the intraday panel.
//
// Plain C++, workgroup barriers only, each reached by every thread of its workgroup.  A (window, prior) result depends on the
// window's C, T, t and row count, on its own prior and on k alone: every sum below runs in an order fixed by k.
#include "posterior_tiled_sweep_prims.h"
#include "posterior_prior_sweep.h"

namespace {

__global__ void __launch_bounds__(NTHREADS) prior_sweep_tiled_fill_kernel(const tp_prior_sweep_tiled_kargs_t A, const tp_tiled_ws_t ws) {
    __shared__ double tc[SB][SB + 1];          // the tile of C (zero outside k x k)
    __shared__ double wI[SB], wJ[SB];          // w0 of the tile's rows / columns (zero beyond k)
    __shared__ double red[2][4][SB];           // 16-term pieces of the row / column products
    const int tid = threadIdx.x;
    const int k = A.k, KP = ws.KP, NS = ws.NS;
    long long e;
    int I, J;
    if (!xcd_entry_tile(NS, A.e_count, e, I, J)) return;
    const long long f = A.e_first + e;         // flat (window, prior) index
    const long long w = f / A.P;
    const long long wl = w - A.wc_first;
    const double* __restrict__ C = A.C + wl * (long long)k * k;
    const double* __restrict__ T = A.T + wl * (long long)k * k;
    const double* __restrict__ w0 = A.w0 + f * k;
    const double ap = prior_scale(A.n0[f], hf_rows(A, w));
    double* M = ws.arena + e * (long long)KP * KP;

    if (tid < SB) wI[tid] = SB * I + tid < k ? w0[SB * I + tid] : 0.0;
    else if (tid < 2 * SB) wJ[tid - SB] = SB * J + (tid - SB) < k ? w0[SB * J + (tid - SB)] : 0.0;
    const int c = tid & (SB - 1), q = tid >> 6;
    const int gj = SB * J + c;
    for (int r = q; r < SB; r += NTHREADS / SB) {
        const int gi = SB * I + r;
        const bool in = gi < k && gj < k;
        const double cv = in ? C[(long long)gi * k + gj] : 0.0;
        const double tv = in ? T[(long long)gi * k + gj] : 0.0;
        const double border = (gj == k && gi < k) ? A.t[w * k + gi] : 0.0;
        M[(long long)gi * KP + gj] = in ? fma(ap, cv, tv) : border;
        tc[r][c] = cv;
    }
    __syncthreads();
    // thread (c, q): quarter q of row c's product with the columns' w0 and of column c's product with the rows' w0
    double sr, sc;
    tile_products16<false>(tc, wI, wJ, c, q, I, J, k, sr, sc);
    red[0][q][c] = sr;
    red[1][q][c] = sc;
    __syncthreads();
    double* part = ws.part + e * (long long)NS * NS * SB;
    if (tid < SB)
        part[((long long)I * NS + J) * SB + tid] = ap * sum4(red[0][0][tid], red[0][1][tid], red[0][2][tid], red[0][3][tid]);
    else if (tid < 2 * SB && I < J) {
        const int l = tid - SB;
        part[((long long)J * NS + I) * SB + l] = ap * sum4(red[1][0][l], red[1][1][l], red[1][2][l], red[1][3][l]);
    }
}

__global__ void __launch_bounds__(NTHREADS) prior_sweep_tiled_border_kernel(const tp_prior_sweep_tiled_kargs_t A, const tp_tiled_ws_t ws) {
    const long long e = blockIdx.x;
    const long long f = A.e_first + e;
    // v0: scratch of this entry (a run keeps its column means here)
    const EntryScal sc = conj_border(ws, e, A.k, ws.part + e * (long long)ws.NS * ws.NS * SB, A.w0 + f * A.k, A.n0 + f, hf_rows(A, f / A.P),
                                     ws.ybar + e * ws.KP);
    close_entry(ws, e, A.k, sc);
}

}  // namespace

hipError_t tp_prior_sweep_tiled_launch(const tp_prior_sweep_tiled_kargs_t& a, const tp_tiled_ws_t& ws, hipStream_t stream) {
    if (a.k < 1 || a.P < 1 || a.e_count < 1 || a.e_count > 65535 || ws.part == nullptr) return hipErrorInvalidValue;
    hipLaunchKernelGGL(prior_sweep_tiled_fill_kernel, xcd_entry_grid(ws.NS, a.e_count), dim3(NTHREADS), 0, stream, a, ws);
    hipLaunchKernelGGL(prior_sweep_tiled_border_kernel, dim3((unsigned)a.e_count), dim3(NTHREADS), 0, stream, a, ws);
    return hipGetLastError();
}
