// posterior_size_sweep_tiled.hip - size sweep above the LDS solve core (tp_batch_size_sweep_tiled, k > tp_sweep_max_assets()):
// S nested universes per window - the first k_1 < ... < k_S <= k columns - from ONE pair of Grams and ONE factorisation at k
// by the large-k tiled pipeline.
//
// The Gram stage of the tiled path (tp_tiled_gram_launch, steered by its arguments: tangency_sweep.cpp) has stored, per window
// of the sub-range, T = X'X, C = Y'Y - (Y'1)(Y'1)'/m and t = X'1 (Jeffreys: M and t as the batch's own strategy forms them).
// An ARENA ENTRY is one (window, prior) pair in a workspace of the solve sweep's geometry for R = S, KP = 64 ceil((k + S)/64),
// NS = KP/64, NSB = ceil(k/64): column k + s holds the right-hand side of size s on rows < k_s and exact zeros below.  The
// block steps (tp_tiled_block_steps_launch) carry every column >= k along and leave it as R^-T column; entry i of a
// forward-substituted column depends on rows <= i only, so rows < k_s of column k + s are the forward substitution of the
// PREFIX system - what the column holds in rows >= k_s is never read.  With a = n0 m/(m-1), size s with k_s columns:
//     v = C[:k_s,:k_s] w0_s     q0 = a w0_s'v     c = 2 n0 / (g + sqrt(g^2 + 4 n0 q0)),  g = n0 + k_s + 2          (ref:415-418)
//     w1 = S1[:k_s,:k_s]^-1 (c a v + t[:k_s])     q1 = |R^-T rhs|^2     weights = (n1 + k_s + 2) w1 / (n1 - q1) / gamma
//
//   size_sweep_tiled_fill_kernel     one workgroup per (entry, super-tile (I, J), I <= J): a C + T (Jeffreys: M) inside k x k,
//                                    zero elsewhere (Jeffreys: t on rows < k_s of column k + s), the flag cleared; conjugate:
//                                    per size with 64 J < k_s the 64-row pieces of C[:k_s,:k_s] w0_s the tile contributes
//                                    (rows of I from the columns of J and, I < J, rows of J from the columns of I)
//   size_sweep_tiled_border_kernel   conjugate, one workgroup per (entry, size): v_s from the pieces of the ceil(k_s/64)
//                                    column blocks in their order, q0_s, c_s, c_s a v_s + t into rows < k_s of column k + s
//   size_sweep_tiled_solve_kernel    one workgroup per entry, sizes in groups of up to 4: q1_s, the blocked back substitution
//                                    of the prefix systems (back_substitute<G, true>), rescale, aux, status
//
// The grid decode, the conjugate scalars, the tile products, the piece sums, the back substitution with its group dispatch and
// LDS size, and the pivot floor are posterior_tiled_sweep_prims.h's.
//
// Whatever lies at or beyond a prefix is excluded by a SELECT, never by a multiplication with zero: w0 and C beyond k_s, the
// factor's columns >= k_s and the inverse block's entries at or beyond p (which may be Inf or NaN) do not reach size s through
// these kernels.  The block steps between them multiply whole 64-row blocks by R_jj^-T with MFMAs, where a structural zero times
// a NaN is a NaN: a NON-FINITE column j spoils the sizes in (64 floor(j/64), j] too - they come back flagged -, which the LDS
// size sweep keeps (include/tangency_posterior.h).  A finite degenerate column j leaves every k_s <= j intact.
//
// Status per size: NOT_PD when some i < k_s has d_i <= k_s 2^-52 M_ii, d_i = 1/(R^-1)_ii^2 from the inverse diagonal blocks,
// M_ii = a C_ii + T_ii (a NaN fails the comparison).  The entry's flag in ws.flags speaks of the pivots of the whole k and
// decides no size.  Then NONFINITE, then BAD_DENOM (conjugate).
//
// C is RAW-MOMENT centred as in the tiled prior sweep (posterior_prior_sweep_tiled.hip): exact to rounding
// for returns, it loses digits under a large common offset of the intraday panel.
//
// Plain C++, workgroup barriers only, each reached by every thread of its workgroup.  A (window, prior, size) result depends on
// the window's matrices, on its own prior and on k, k_s and the workspace's geometry alone: every sum below runs in an order
// fixed by k and k_s, and a size's arithmetic does not depend on which other sizes share its group.
#include "posterior_tiled_sweep_prims.h"
#include "posterior_size_sweep_tiled.h"

namespace {

constexpr int MAXS = TP_SWEEP_KMAX_RHS;        // sizes per sweep

// a = n0 m/(m-1) of the flat (window, prior) index f
__device__ __forceinline__ double entry_scale(const tp_size_sweep_tiled_kargs_t& A, const long long f) {
    return prior_scale(A.n0[f], hf_rows(A, f / A.P));
}

template <bool CONJ>
__global__ void __launch_bounds__(NTHREADS) size_sweep_tiled_fill_kernel(const tp_size_sweep_tiled_kargs_t A, const tp_tiled_ws_t ws) {
    __shared__ double tc[CONJ ? SB : 1][SB + 1];            // the tile of C
    __shared__ double wI[CONJ ? MAXS : 1][SB], wJ[CONJ ? MAXS : 1][SB];     // w0_s of the tile's rows / columns (zero beyond k_s)
    const int tid = threadIdx.x;
    const int k = A.k, S = A.S, KP = ws.KP, NS = ws.NS, NSB = ws.NSB;
    long long e;
    int I, J;
    if (!xcd_entry_tile(NS, A.e_count, e, I, J)) return;
    const long long f = A.e_first + e;         // flat (window, prior) index
    const long long w = f / A.P;
    const long long wl = w - A.wc_first;
    const double* __restrict__ T = A.T + wl * (long long)k * k;
    const double* __restrict__ C = CONJ ? A.C + wl * (long long)k * k : nullptr;
    const double ap = CONJ ? entry_scale(A, f) : 0.0;
    double* M = ws.arena + e * (long long)KP * KP;
    const int c = tid & (SB - 1), q = tid >> 6;
    const int gj = SB * J + c;                  // < KP
    // Jeffreys: column k + s holds t on rows < k_s (the conjugate right-hand sides are the border kernel's)
    int kcol = 0;
    if (!CONJ && gj >= k && gj - k < S) kcol = A.sizes[gj - k];
    for (int r = q; r < SB; r += NTHREADS / SB) {
        const int gi = SB * I + r;              // < KP
        const bool in = gi < k && gj < k;
        double v = 0.0;                         // rows >= k, columns >= k + S, rows >= k_s of a right-hand side
        if constexpr (CONJ) {
            const double cv = in ? C[(long long)gi * k + gj] : 0.0;
            if (in) v = fma(ap, cv, T[(long long)gi * k + gj]);
            tc[r][c] = cv;
        } else {
            if (in) v = T[(long long)gi * k + gj];
            else if (gi < kcol) v = A.t[w * k + gi];
        }
        M[(long long)gi * KP + gj] = v;
    }
    if (J == 0 && tid == 0) ws.flags[e] = 0;       // (super-tile (0, 0))
    if constexpr (CONJ) {
        const double* __restrict__ w0 = A.w0 + f * (long long)S * k;
        for (int x = tid; x < 2 * SB * S; x += NTHREADS) {
            const int s = x / (2 * SB), l = x & (SB - 1);
            const bool isJ = (x & SB) != 0;
            const int g = SB * (isJ ? J : I) + l;
            const double v = g < A.sizes[s] ? w0[(long long)s * k + g] : 0.0;      // never read at or beyond k_s
            if (isJ) wJ[s][l] = v; else wI[s][l] = v;
        }
        __syncthreads();
        // wavefront q takes sizes q, q + 4, ...; lane c: row c's product with the columns' w0_s and column c's with the rows'.
        // Terms at or beyond k_s are selected out, not multiplied by zero (tile_products16<true>).
        double* part = ws.part + e * (long long)S * NSB * NSB * SB;
        for (int s = q; s < S; s += NTHREADS / SB) {
            const int ks = A.sizes[s];
            if (SB * J >= ks) continue;         // (no barrier below) the tile lies outside the prefix: the border reads none of it
            double pr[4], pc[4];
#pragma unroll
            for (int h = 0; h < 4; ++h) tile_products16<true>(tc, wI[s], wJ[s], c, h, I, J, ks, pr[h], pc[h]);
            part[(((long long)s * NSB + I) * NSB + J) * SB + c] = sum4(pr);
            if (I < J) part[(((long long)s * NSB + J) * NSB + I) * SB + c] = sum4(pc);
        }
    }
}

__global__ void __launch_bounds__(NTHREADS) size_sweep_tiled_border_kernel(const tp_size_sweep_tiled_kargs_t A, const tp_tiled_ws_t ws) {
    const int tid = threadIdx.x;
    const int k = A.k, S = A.S, KP = ws.KP, NSB = ws.NSB;
    const long long e = blockIdx.x / S;
    const int s = (int)(blockIdx.x - e * S);
    const long long f = A.e_first + e;
    const long long w = f / A.P;
    const int ks = A.sizes[s];
    const double* __restrict__ w0 = A.w0 + (f * S + s) * (long long)k;
    const double* part = ws.part + ((e * S + s) * (long long)NSB * NSB) * SB;
    double* col = ws.arena + e * (long long)KP * KP + (k + s);
    // v_s into the column (rewritten below by the thread that wrote it) from the ceil(k_s/64) column blocks' pieces
    const double wv = pieces_dot(part, NSB, (ks + SB - 1) / SB, ks, w0, col, KP);
    const double n0 = A.n0[f];
    const double ap = entry_scale(A, f);
    const double q0 = ap * wv;
    const double cc = shrink_c(n0, ks, q0);
    const double ca = cc * ap;
    for (int i = tid; i < ks; i += NTHREADS) col[(long long)i * KP] = fma(ca, col[(long long)i * KP], A.t[w * k + i]);
    if (tid == 0) {
        double* ax = A.aux + (f * S + s) * 8;   // (the solve kernel writes the other slots)
        ax[2] = cc; ax[3] = q0;
    }
}

// sizes g0 .. g0 + G - 1 of one entry: wvec [G][KP] | zv [G][64]; qs, lowm, badm: per member of the group
template <int G, bool CONJ>
__device__ __forceinline__ void solve_group(const tp_size_sweep_tiled_kargs_t& A, const tp_tiled_ws_t& ws, const long long e,
                                            const int g0, double* wvec, double* zv, double (*qs)[4], int* lowm, int* badm) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int k = A.k, S = A.S, KP = ws.KP, NSB = ws.NSB;
    const double* M = ws.arena + e * (long long)KP * KP;
    const long long f = A.e_first + e;
    int ks[G];
#pragma unroll
    for (int g = 0; g < G; ++g) ks[g] = A.sizes[g0 + g];
    if (tid < G) { lowm[tid] = 0; badm[tid] = 0; }
    // q1_s = y'y over the prefix, y = the forward-substituted column
#pragma unroll
    for (int g = 0; g < G; ++g) {
        double qv = 0.0;
        for (int i = tid; i < ks[g]; i += NTHREADS) { const double y = M[(long long)i * KP + k + g0 + g]; qv = fma(y, y, qv); }
        qv = wave_sum64(qv);
        if (lane == 0) qs[g][wv] = qv;
    }
    __syncthreads();
    back_substitute<G, true>(M, KP, k, NSB, k + g0, ws.rinv, e * NSB, ks, wvec, zv);
    // the floor of the pivots inside the prefix, the rescale and the weights
    const double n0 = CONJ ? A.n0[f] : 0.0;
    const double ap = CONJ ? entry_scale(A, f) : 0.0;
    const double n1 = n0 + (double)A.N;
    const double inv_gamma = 1.0 / A.gamma;
    const long long wl = f / A.P - A.wc_first;
    const double* __restrict__ T = A.T + wl * (long long)k * k;
    const double* __restrict__ C = CONJ ? A.C + wl * (long long)k * k : nullptr;
    const double* rinv0 = ws.rinv + e * NSB * (long long)(SB * SB);
    double denom[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const double q1 = sum4(qs[g]);
        denom[g] = n1 - q1;
        bool bad = false;
        const bool low = low_pivot(rinv0, ks[g], [&](const int i) {
            const long long ii = (long long)i * k + i;
            return CONJ ? fma(ap, C[ii], T[ii]) : T[ii];
        });
        double* out = A.weights + ((f * S + g0 + g) * (long long)k);
        for (int i = tid; i < k; i += NTHREADS) {
            double v = 0.0;                                          // exact zeros beyond the prefix
            if (i < ks[g]) {
                const double wi = wvec[g * KP + i];
                v = CONJ ? inv_gamma * ((n1 + ks[g] + 2) * wi / denom[g]) : wi * inv_gamma;
                if (!isfinite(v)) bad = true;
            }
            out[i] = v;
        }
        if (low) lowm[g] = 1;
        if (bad) badm[g] = 1;
    }
    __syncthreads();
    if (tid < G) {
        const int g = tid;
        const double q1 = sum4(qs[g]);
        const double den = n1 - q1;
        int st = TP_KSTATUS_OK;
        if (lowm[g]) st = TP_KSTATUS_NOT_PD;
        else if (badm[g]) st = TP_KSTATUS_NONFINITE;
        else if (CONJ && !(den > 0.0)) st = TP_KSTATUS_BAD_DENOM;
        A.status[f * S + g0 + g] = st;
        double* ax = A.aux + (f * S + g0 + g) * 8;
        ax[0] = n0; ax[1] = CONJ ? n1 : 0.0;
        if (!CONJ) { ax[2] = 0.0; ax[3] = 0.0; }   // (conjugate: c and q0 are the border kernel's)
        ax[4] = q1; ax[5] = CONJ ? den : 0.0; ax[6] = 0.0; ax[7] = 0.0;
    }
    __syncthreads();                               // the next group overwrites wvec, qs and the marks
}

template <bool CONJ>
__global__ void __launch_bounds__(NTHREADS) size_sweep_tiled_solve_kernel(const tp_size_sweep_tiled_kargs_t A, const tp_tiled_ws_t ws) {
    extern __shared__ __attribute__((aligned(16))) double sm[];     // wvec [min(S, NG)][KP] | zv [NG][64]
    __shared__ double qs[NG][4];
    __shared__ int lowm[NG], badm[NG];
    const long long e = blockIdx.x;
    const int S = A.S;
    double* wvec = sm;
    double* zv = sm + (S < NG ? S : NG) * ws.KP;
    for_each_group(S, [&](auto G, const int g0) { solve_group<decltype(G)::value, CONJ>(A, ws, e, g0, wvec, zv, qs, lowm, badm); });
}

bool args_fit(const tp_size_sweep_tiled_kargs_t& a, const tp_tiled_ws_t& ws) {
    return a.k >= 1 && a.P >= 1 && a.S >= 1 && a.S <= MAXS && a.e_count >= 1 && a.e_count <= 65535 && a.k + a.S <= ws.KP &&
           ws.KP == SB * ws.NS && ws.KP <= 32 * SB && ws.NSB == (a.k + SB - 1) / SB && a.T != nullptr && a.sizes != nullptr &&
           (a.C == nullptr || (ws.part != nullptr && a.n0 != nullptr && a.w0 != nullptr));
}

}  // namespace

size_t tp_size_sweep_tiled_part_doubles(int k, int S) {
    const size_t nsb = (size_t)(k + SB - 1) / SB;
    return (size_t)S * nsb * nsb * SB;
}

hipError_t tp_size_sweep_tiled_fill_launch(const tp_size_sweep_tiled_kargs_t& a, const tp_tiled_ws_t& ws, hipStream_t stream) {
    if (!args_fit(a, ws)) return hipErrorInvalidValue;
    const dim3 grid = xcd_entry_grid(ws.NS, a.e_count);
    if (a.C != nullptr) {
        hipLaunchKernelGGL(size_sweep_tiled_fill_kernel<true>, grid, dim3(NTHREADS), 0, stream, a, ws);
        hipLaunchKernelGGL(size_sweep_tiled_border_kernel, dim3((unsigned)(a.e_count * a.S)), dim3(NTHREADS), 0, stream, a, ws);
    } else {
        hipLaunchKernelGGL(size_sweep_tiled_fill_kernel<false>, grid, dim3(NTHREADS), 0, stream, a, ws);
    }
    return hipGetLastError();
}

hipError_t tp_size_sweep_tiled_solve_launch(const tp_size_sweep_tiled_kargs_t& a, const tp_tiled_ws_t& ws, hipStream_t stream) {
    if (!args_fit(a, ws)) return hipErrorInvalidValue;
    size_t smem;
    static std::atomic<unsigned long long> attr_done[2];      // one bit per device (tp_allow_dynamic_lds), one word per kernel
    if (a.C != nullptr) {
        const hipError_t e = group_solve_lds(attr_done[0], size_sweep_tiled_solve_kernel<true>, a.S, ws.KP, &smem);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(size_sweep_tiled_solve_kernel<true>, dim3((unsigned)a.e_count), dim3(NTHREADS), smem, stream, a, ws);
    } else {
        const hipError_t e = group_solve_lds(attr_done[1], size_sweep_tiled_solve_kernel<false>, a.S, ws.KP, &smem);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(size_sweep_tiled_solve_kernel<false>, dim3((unsigned)a.e_count), dim3(NTHREADS), smem, stream, a, ws);
    }
    return hipGetLastError();
}
