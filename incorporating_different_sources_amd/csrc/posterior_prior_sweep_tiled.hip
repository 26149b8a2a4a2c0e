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
//   prior_sweep_tiled_border_kernel   one workgroup per entry: v = a C w0 from the pieces in a fixed order, q0 = w0'v,
//                                     c (ref:415-418), c v added to column k, ws.scal = (s, sqrt s, c, q0, n0), rows >= k
//                                     and the flag zeroed - the arithmetic of tiled_clear_kernel's shared-intraday branch
//
// C is RAW-MOMENT centred (the Gram kernels' row-count centring, center_rows = 1), not shifted by a row of the window like the
// run kernels' S0: exact to rounding while the intraday mean is small against the spread (returns), it loses digits under a
// large common offset of the intraday panel.
//
// Plain C++, workgroup barriers only, each reached by every thread of its workgroup.  A (window, prior) result depends on the
// window's C, T, t and row count, on its own prior and on k alone: every sum below runs in an order fixed by k.
#include "posterior_device_prims.h"
#include "posterior_prior_sweep.h"

namespace {

constexpr int SB = 64;
constexpr int NTHREADS = 256;

__global__ void __launch_bounds__(NTHREADS) prior_sweep_tiled_fill_kernel(const tp_prior_sweep_tiled_kargs_t A, const tp_tiled_ws_t ws) {
    __shared__ double tc[SB][SB + 1];          // the tile of C (zero outside k x k)
    __shared__ double wI[SB], wJ[SB];          // w0 of the tile's rows / columns (zero beyond k)
    __shared__ double red[2][4][SB];           // 16-term pieces of the row / column products
    const int tid = threadIdx.x;
    const int k = A.k, KP = ws.KP, NS = ws.NS;
    const int NT = NS * (NS + 1) / 2;
    // The tiled path's grid decode (workgroup id -> XCD = id % 8, slot = id / 8; tiles of an entry consecutive on one XCD),
    // with the entries dealt to the XCDs in eight contiguous runs: the P entries of a window follow each other on ONE XCD,
    // whose L2 then serves their reads of the window's C and T.
    const long long id = blockIdx.x;
    const long long slot = id >> 3;
    const long long per_xcd = (A.e_count + 7) / 8;
    const long long e = (id & 7) * per_xcd + slot / NT;
    if (e >= A.e_count) return;                 // (uniform per workgroup, in front of every barrier)
    const int tile = (int)(slot % NT);
    int I, J;
    pair_decode(tile, NS, I, J);
    const long long f = A.e_first + e;         // flat (window, prior) index
    const long long w = f / A.P;
    const long long wl = w - A.wc_first;
    const double* __restrict__ C = A.C + wl * (long long)k * k;
    const double* __restrict__ T = A.T + wl * (long long)k * k;
    const double* __restrict__ w0 = A.w0 + f * k;
    const double n0 = A.n0[f];
    const double mm = (double)(A.hf_count != nullptr ? A.hf_count[w] : A.m);
    const double ap = n0 * (mm / (mm - 1.0));                  // ref:333, as the run kernels form it
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
    // thread (c, q): 16 terms of row c's product with the columns' w0 and of column c's product with the rows' w0
    double sr = 0.0, sc = 0.0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        sr = fma(tc[c][16 * q + i], wJ[16 * q + i], sr);
        sc = fma(tc[16 * q + i][c], wI[16 * q + i], sc);
    }
    red[0][q][c] = sr;
    red[1][q][c] = sc;
    __syncthreads();
    double* part = ws.part + e * (long long)NS * NS * SB;
    if (tid < SB)
        part[((long long)I * NS + J) * SB + tid] = ap * (((red[0][0][tid] + red[0][1][tid]) + red[0][2][tid]) + red[0][3][tid]);
    else if (tid < 2 * SB && I < J) {
        const int l = tid - SB;
        part[((long long)J * NS + I) * SB + l] = ap * (((red[1][0][l] + red[1][1][l]) + red[1][2][l]) + red[1][3][l]);
    }
}

__global__ void __launch_bounds__(NTHREADS) prior_sweep_tiled_border_kernel(const tp_prior_sweep_tiled_kargs_t A, const tp_tiled_ws_t ws) {
    __shared__ double red[4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const long long e = blockIdx.x;
    const int k = A.k, KP = ws.KP, NS = ws.NS;
    const long long f = A.e_first + e;
    const long long w = f / A.P;
    const double* __restrict__ w0 = A.w0 + f * k;
    double* M = ws.arena + e * (long long)KP * KP;
    const double* part = ws.part + e * (long long)NS * NS * SB;
    double* v0 = ws.ybar + e * KP;             // scratch of this entry (a run keeps its column means here)
    double qq = 0.0;
    for (int i = tid; i < k; i += NTHREADS) {
        const double* pp = part + ((long long)(i >> 6) * NS) * SB + (i & 63);
        double v = 0.0;
        for (int src = 0; src < NS; ++src) v += pp[src * SB];
        v0[i] = v;
        qq = fma(w0[i], v, qq);
    }
    qq = wave_sum64(qq);
    if (lane == 0) red[wv] = qq;
    __syncthreads();
    const double q0 = ((red[0] + red[1]) + red[2]) + red[3];
    const double n0 = A.n0[f];
    const double mm = (double)(A.hf_count != nullptr ? A.hf_count[w] : A.m);
    const double s = n0 * (mm / (mm - 1.0));
    const double a = n0 + k + 2;
    const double c = (2 * n0) / (a + sqrt(a * a + 4 * n0 * q0));       // ref:415-418
    for (int i = tid; i < k; i += NTHREADS) M[(long long)i * KP + k] += c * v0[i];
    if (tid == 0) {
        double* o = ws.scal + e * 8;
        o[0] = s; o[1] = sqrt(s); o[2] = c; o[3] = q0; o[4] = n0;
        ws.flags[e] = 0;
    }
    // rows >= k of the bordered matrix are never pivots (tiled_clear_kernel)
    for (int x = tid; x < (KP - k) * KP; x += NTHREADS) M[(long long)k * KP + x] = 0.0;
}

}  // namespace

hipError_t tp_prior_sweep_tiled_launch(const tp_prior_sweep_tiled_kargs_t& a, const tp_tiled_ws_t& ws, hipStream_t stream) {
    if (a.k < 1 || a.P < 1 || a.e_count < 1 || a.e_count > 65535 || ws.part == nullptr) return hipErrorInvalidValue;
    const long long NT = (long long)ws.NS * (ws.NS + 1) / 2;
    const long long grid = ((a.e_count + 7) / 8) * 8 * NT;
    hipLaunchKernelGGL(prior_sweep_tiled_fill_kernel, dim3((unsigned)grid), dim3(NTHREADS), 0, stream, a, ws);
    hipLaunchKernelGGL(prior_sweep_tiled_border_kernel, dim3((unsigned)a.e_count), dim3(NTHREADS), 0, stream, a, ws);
    return hipGetLastError();
}
