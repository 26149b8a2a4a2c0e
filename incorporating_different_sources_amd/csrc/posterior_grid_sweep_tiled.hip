// posterior_grid_sweep_tiled.hip - grid sweep above the LDS solve core (tp_batch_grid_sweep_tiled, k > tp_sweep_max_assets()):
// S nested universes x L nested window lengths per window from ONE pass over the rows of the longest window at the largest size
// and ONE factorisation per (window, prior, length) by the large-k tiled pipeline.
//
// The two halves exist above tp_sweep_max_assets() and compose.  Suffix half (posterior_window_sweep_tiled.hip): per window of
// the sub-range the Gram stage has stored, conjugate, C = Y'Y - (Y'1)(Y'1)'/m (symmetric, full storage: the batch's own tiled
// Gram stage over the intraday rows), per length the snapshot G_l = sum x x' (column >= row) and g_l = sum x over the length's
// suffix (the segmented one-wave Gram), and with a delta the sums v, s1, s2 of the rank-two correction.  Prefix half
// (posterior_size_sweep_tiled.hip): an ARENA ENTRY - here one (window, prior, length), flat index (w P + p) L + l - lives in a
// workspace of the solve sweep's geometry for R = S, KP = 64 ceil((k + S)/64), NS = KP/64, NSB = ceil(k/64); column k + s holds
// the right-hand side of size s on rows < k_s and exact zeros below; the block steps (tp_tiled_block_steps_launch) carry every
// column >= k along, and rows < k_s of column k + s come out as the forward substitution of the PREFIX system.  With
// T = G_l - v 1' - 1 v' + s2 1 1' evaluated left to right (v = 0, s1 = s2 = 0: the bits of G_l), t = g_l - s1 1 and, conjugate,
// a = n0_wpl m/(m-1), size s with k_s columns:
//     v_s = C[:k_s,:k_s] w0_wps[:k_s]     q0 = a w0_wps'v_s     c = 2 n0 / (g + sqrt(g^2 + 4 n0 q0)),  g = n0_wpl + k_s + 2
//     w1 = (a C + T)[:k_s,:k_s]^-1 (c a v_s + t[:k_s])     q1 = |R^-T rhs|^2     weights = (n1 + k_s + 2) w1 / (n1 - q1) / gamma,
//     n1 = n0_wpl + N_l;     Jeffreys: M = T - t t'/N_l (TP_FLAG_CENTER_BY_ROWS: / rows_wl, TP_FLAG_NO_CENTER: no term), weights = M[:k_s,:k_s]^-1 t[:k_s] / gamma
//
//   grid_sweep_tiled_cw_kernel     conjugate, one workgroup per (window, prior) of the sub-range: ONE pass over the rows of C forms
//                                  the S truncated products v_s and w0_wps'v_s - they depend on neither the length nor n0
//   grid_sweep_tiled_fill_kernel   one workgroup per (entry, super-tile (I, J), I <= J): the matrix inside k x k, the S right-hand
//                                  sides, zero elsewhere, the flag cleared; the diagonal super-tiles keep the diagonal they write
//                                  (mdiag), super-tile (0, 0) puts c_s and q0_s into the entry's aux rows
//   grid_sweep_tiled_solve_kernel  one workgroup per entry, sizes in groups of up to 4: q1_s, the blocked back substitution of the
//                                  prefix systems (back_substitute<G, true>), rescale with N[l] and n0_wpl of the ENTRY, weights,
//                                  aux and status straight to slot ((w P + p) L + l) S + s
//
// The solve reads N per entry, so the entries of a group need not share a length: all lengths of a sub-range go through the
// block steps together.  The grid decode, the conjugate scalars, the back substitution with its group dispatch and LDS size, and
// the pivot floor are posterior_tiled_sweep_prims.h's.
//
// Whatever lies at or beyond a prefix is excluded by a SELECT, never by a multiplication with zero, as in the tiled size sweep;
// the block steps multiply whole 64-row blocks with MFMAs, so a NON-FINITE column j spoils the sizes in (64 floor(j/64), j] too -
// they come back flagged.  A finite degenerate column j leaves every k_s <= j intact.
//
// Status per size: NOT_PD when some i < k_s has d_i <= k_s 2^-52 M_ii, d_i = 1/(R^-1)_ii^2 from the inverse diagonal blocks,
// M_ii as the fill stored it (a NaN fails the comparison).  The entry's flag in ws.flags speaks of the pivots of the whole k and
// decides no size.  Then NONFINITE, then BAD_DENOM (conjugate).
//
// Plain C++, workgroup barriers only, each reached by every thread of its workgroup; every loop is bounded by k, KP or the
// launch's arguments.  An entry's result depends on the window's C, its own snapshot and delta sums, its prior, N_l, k, k_s and
// the workspace's geometry alone: every sum below runs in an order fixed by k and k_s.
#include "posterior_tiled_sweep_prims.h"
#include "posterior_grid_sweep_tiled.h"

namespace {

constexpr int MAXS = TP_SWEEP_KMAX_RHS;        // sizes per sweep

// MS: the sizes the accumulators are unrolled over (4 ceil(S/4) up to 8, else 16); RB: rows of C per wavefront and pass, which
// share the loads of w0.  The operations on a (row, size) and their order are the same in every instantiation: lane l takes the
// columns l, l + 64, ... < k_s of the row in this order, then the wave sum.
template <int MS, int RB>
__global__ void __launch_bounds__(NTHREADS) grid_sweep_tiled_cw_kernel(const tp_grid_sweep_tiled_kargs_t A) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int k = A.k, S = A.S;
    const long long wp = A.wp_first + blockIdx.x;
    const long long w = wp / A.P;
    const long long wpl = wp - A.wc_first * A.P;               // the pair's number inside the sub-range
    const double* __restrict__ C = A.C + (w - A.wc_first) * (long long)k * k;
    const double* __restrict__ w0 = A.w0 + wp * (long long)S * k;
    double* cv = A.cv + wpl * (long long)S * k;
    int ks[MS];
#pragma unroll
    for (int s = 0; s < MS; ++s) ks[s] = s < S ? A.sizes[s] : 0;
    const int kmax = A.sizes[S - 1];
    for (int i0 = wv * RB; i0 < kmax; i0 += (NTHREADS / 64) * RB) {
        double acc[RB][MS];
        const double* __restrict__ row[RB];
#pragma unroll
        for (int r = 0; r < RB; ++r) {
            // (a row at or beyond kmax is not stored: the last row stands in for its loads)
            row[r] = C + (long long)(i0 + r < kmax ? i0 + r : kmax - 1) * k;
#pragma unroll
            for (int s = 0; s < MS; ++s) acc[r][s] = 0.0;
        }
        for (int c = lane; c < kmax; c += 64) {
            double cr[RB];
#pragma unroll
            for (int r = 0; r < RB; ++r) cr[r] = row[r][c];
#pragma unroll
            for (int s = 0; s < MS; ++s)
                if (c < ks[s]) {                                // selected out beyond k_s, never multiplied by zero
                    const double wc = w0[(long long)s * k + c];
#pragma unroll
                    for (int r = 0; r < RB; ++r) acc[r][s] = fma(cr[r], wc, acc[r][s]);
                }
        }
#pragma unroll
        for (int s = 0; s < MS; ++s) {
            if (s < S) {                                        // (uniform per workgroup)
#pragma unroll
                for (int r = 0; r < RB; ++r) {
                    const double v = wave_sum64(acc[r][s]);
                    if (lane == 0 && i0 + r < ks[s]) cv[(long long)s * k + i0 + r] = v;
                }
            }
        }
    }
    __syncthreads();
    // w0_s'v_s: wavefront wv takes the sizes wv, wv + 4, ...
    for (int s = wv; s < S; s += NTHREADS / 64) {
        const int kp = A.sizes[s];
        double q = 0.0;
        for (int i = lane; i < kp; i += 64) q = fma(w0[(long long)s * k + i], cv[(long long)s * k + i], q);
        q = wave_sum64(q);
        if (lane == 0) A.cq[wpl * S + s] = q;
    }
}

// the flat entry index f = (w P + p) L + l taken apart
struct EntryId { long long f, wp, w; int l; };
__device__ __forceinline__ EntryId entry_id(const tp_grid_sweep_tiled_kargs_t& A, const long long e) {
    EntryId id;
    id.f = A.e_first + e;
    id.wp = id.f / A.L;
    id.l = (int)(id.f - id.wp * A.L);
    id.w = id.wp / A.P;
    return id;
}

template <bool CONJ>
__global__ void __launch_bounds__(NTHREADS) grid_sweep_tiled_fill_kernel(const tp_grid_sweep_tiled_kargs_t A, const tp_tiled_ws_t ws) {
    __shared__ double tI[SB], tJ[SB], dI[SB], dJ[SB];          // t = g_l - s1 and the delta kernel's v of the tile's rows / columns
    const int tid = threadIdx.x;
    const int k = A.k, S = A.S, KP = ws.KP, NS = ws.NS, L = A.L;
    long long e;
    int I, J;
    if (!xcd_entry_tile(NS, A.e_count, e, I, J)) return;
    const EntryId id = entry_id(A, e);
    const long long wl = id.w - A.wc_first;
    const long long wlen = id.w * L + id.l;
    const double* __restrict__ T = A.T + (wl * L + id.l) * (long long)k * k;
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
    const int c = tid & (SB - 1), q = tid >> 6;
    const int gj = SB * J + c;                  // < KP
    const double* __restrict__ C = nullptr;
    const double* __restrict__ vs = nullptr;   // v_s of the thread's right-hand-side column
    double ap = 0.0, ca = 0.0, rinv = 0.0;
    int kcol = 0;                               // k_s of the thread's column when it is a right-hand side, else 0
    if (gj >= k && gj - k < S) kcol = A.sizes[gj - k];
    if constexpr (CONJ) {
        const long long pair = id.wp - A.wc_first * A.P;
        const double n0 = A.n0[id.f];
        ap = prior_scale(n0, hf_rows(A, id.w));
        C = A.C + wl * (long long)k * k;
        if (kcol > 0) {
            const int s = gj - k;
            vs = A.cv + (pair * S + s) * (long long)k;
            ca = shrink_c(n0, kcol, ap * A.cq[pair * S + s]) * ap;
        }
        if (I == 0 && J == 0 && tid < S) {     // c_s and q0_s of the entry: the solve writes the other slots
            const double q0 = ap * A.cq[pair * S + tid];
            double* ax = A.aux + (id.f * S + tid) * 8;
            ax[2] = shrink_c(n0, A.sizes[tid], q0); ax[3] = q0;
        }
    } else {
        rinv = A.center_rows == 2 ? 0.0 : 1.0 / (A.center_rows == 1 ? (double)A.rows[wlen] : (double)A.N[id.l]);
    }
    for (int r = q; r < SB; r += NTHREADS / SB) {
        const int gi = SB * I + r;              // < KP
        double out = 0.0;                       // rows >= k, columns >= k + S, rows >= k_s of a right-hand side
        if (gi < k && gj < k) {
            // element (lo, hi) of the upper triangle; a diagonal super-tile mirrors it below its diagonal
            const bool up = I < J || r <= c;
            const int lo = up ? gi : gj, hi = up ? gj : gi;
            const double dlo = up ? dI[r] : dJ[c], dhi = up ? dJ[c] : dI[r];
            const double tv = T[(long long)lo * k + hi] - dlo - dhi + s2;      // G - v 1' - 1 v' + s2 1 1'
            if constexpr (CONJ) {
                out = fma(ap, C[(long long)gi * k + gj], tv);
            } else {
                const double tlo = up ? tI[r] : tJ[c], thi = up ? tJ[c] : tI[r];
                out = A.center_rows == 2 ? tv : fma(-(tlo * rinv), thi, tv);
            }
            if (I == J && r == c) A.mdiag[e * k + gi] = out;
        } else if (gi < kcol) {
            out = CONJ ? fma(ca, vs[gi], tI[r]) : tI[r];
        }
        M[(long long)gi * KP + gj] = out;
    }
    if (I == 0 && J == 0 && tid == 0) ws.flags[e] = 0;
}

// sizes g0 .. g0 + G - 1 of one entry: wvec [G][KP] | zv [G][64]; qs, lowm, badm: per member of the group
template <int G, bool CONJ>
__device__ __forceinline__ void solve_group(const tp_grid_sweep_tiled_kargs_t& A, const tp_tiled_ws_t& ws, const long long e,
                                            const int g0, double* wvec, double* zv, double (*qs)[4], int* lowm, int* badm) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int k = A.k, S = A.S, KP = ws.KP, NSB = ws.NSB;
    const double* M = ws.arena + e * (long long)KP * KP;
    const EntryId id = entry_id(A, e);
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
    // the floor of the pivots inside the prefix, the rescale with the ENTRY's N and n0, and the weights
    const double n0 = CONJ ? A.n0[id.f] : 0.0;
    const double n1 = n0 + (double)A.N[id.l];
    const double inv_gamma = 1.0 / A.gamma;
    const double* rinv0 = ws.rinv + e * NSB * (long long)(SB * SB);
    const double* __restrict__ md = A.mdiag + e * k;
    double denom[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const double q1 = sum4(qs[g]);
        denom[g] = n1 - q1;
        bool bad = false;
        const bool low = low_pivot(rinv0, ks[g], [&](const int i) { return md[i]; });
        double* out = A.weights + ((id.f * S + g0 + g) * (long long)k);
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
        A.status[id.f * S + g0 + g] = st;
        double* ax = A.aux + (id.f * S + g0 + g) * 8;
        ax[0] = n0; ax[1] = CONJ ? n1 : 0.0;
        if (!CONJ) { ax[2] = 0.0; ax[3] = 0.0; }   // (conjugate: c and q0 are the fill kernel's)
        ax[4] = q1; ax[5] = CONJ ? den : 0.0; ax[6] = 0.0; ax[7] = 0.0;
    }
    __syncthreads();                               // the next group overwrites wvec, qs and the marks
}

template <bool CONJ>
__global__ void __launch_bounds__(NTHREADS) grid_sweep_tiled_solve_kernel(const tp_grid_sweep_tiled_kargs_t A, const tp_tiled_ws_t ws) {
    extern __shared__ __attribute__((aligned(16))) double sm[];     // wvec [min(S, NG)][KP] | zv [NG][64]
    __shared__ double qs[NG][4];
    __shared__ int lowm[NG], badm[NG];
    const long long e = blockIdx.x;
    const int S = A.S;
    double* wvec = sm;
    double* zv = sm + (S < NG ? S : NG) * ws.KP;
    for_each_group(S, [&](auto G, const int g0) { solve_group<decltype(G)::value, CONJ>(A, ws, e, g0, wvec, zv, qs, lowm, badm); });
}

bool args_fit(const tp_grid_sweep_tiled_kargs_t& a, const tp_tiled_ws_t& ws) {
    return a.k >= 1 && a.P >= 1 && a.L >= 1 && a.L <= MAXS && a.S >= 1 && a.S <= MAXS && a.e_count >= 1 && a.e_count <= 65535 &&
           a.e_first >= 0 && a.k + a.S <= ws.KP && ws.KP == SB * ws.NS && ws.KP <= 32 * SB && ws.NSB == (a.k + SB - 1) / SB &&
           a.T != nullptr && a.t != nullptr && a.N != nullptr && a.sizes != nullptr && a.rows != nullptr && a.mdiag != nullptr &&
           (a.C == nullptr || (a.n0 != nullptr && a.w0 != nullptr && a.cv != nullptr && a.cq != nullptr));
}

}  // namespace

hipError_t tp_grid_sweep_tiled_cw_launch(const tp_grid_sweep_tiled_kargs_t& a, hipStream_t stream) {
    if (a.k < 1 || a.P < 1 || a.S < 1 || a.S > MAXS || a.wp_count < 1 || a.wp_count > 0x7fffffffLL || a.C == nullptr ||
        a.w0 == nullptr || a.sizes == nullptr || a.cv == nullptr || a.cq == nullptr)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)a.wp_count);
    if (a.S <= 4) hipLaunchKernelGGL((grid_sweep_tiled_cw_kernel<4, 4>), grid, dim3(NTHREADS), 0, stream, a);
    else if (a.S <= 8) hipLaunchKernelGGL((grid_sweep_tiled_cw_kernel<8, 2>), grid, dim3(NTHREADS), 0, stream, a);
    else hipLaunchKernelGGL((grid_sweep_tiled_cw_kernel<16, 1>), grid, dim3(NTHREADS), 0, stream, a);
    return hipGetLastError();
}

hipError_t tp_grid_sweep_tiled_fill_launch(const tp_grid_sweep_tiled_kargs_t& a, const tp_tiled_ws_t& ws, hipStream_t stream) {
    if (!args_fit(a, ws)) return hipErrorInvalidValue;
    const dim3 grid = xcd_entry_grid(ws.NS, a.e_count);
    if (a.C != nullptr) hipLaunchKernelGGL(grid_sweep_tiled_fill_kernel<true>, grid, dim3(NTHREADS), 0, stream, a, ws);
    else hipLaunchKernelGGL(grid_sweep_tiled_fill_kernel<false>, grid, dim3(NTHREADS), 0, stream, a, ws);
    return hipGetLastError();
}

hipError_t tp_grid_sweep_tiled_solve_launch(const tp_grid_sweep_tiled_kargs_t& a, const tp_tiled_ws_t& ws, hipStream_t stream) {
    if (!args_fit(a, ws)) return hipErrorInvalidValue;
    size_t smem;
    static std::atomic<unsigned long long> attr_done[2];      // one bit per device (tp_allow_dynamic_lds), one word per kernel
    if (a.C != nullptr) {
        const hipError_t e = group_solve_lds(attr_done[0], grid_sweep_tiled_solve_kernel<true>, a.S, ws.KP, &smem);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(grid_sweep_tiled_solve_kernel<true>, dim3((unsigned)a.e_count), dim3(NTHREADS), smem, stream, a, ws);
    } else {
        const hipError_t e = group_solve_lds(attr_done[1], grid_sweep_tiled_solve_kernel<false>, a.S, ws.KP, &smem);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(grid_sweep_tiled_solve_kernel<false>, dim3((unsigned)a.e_count), dim3(NTHREADS), smem, stream, a, ws);
    }
    return hipGetLastError();
}
