#pragma once
// posterior_tiled_sweep_prims.h - what the large-k tiled run (posterior_tiled.hip) and the four tiled sweeps
// (posterior_{prior,solve,size,window}_sweep_tiled.hip) share above the device primitives: the workgroup id -> (entry,
// super-tile) decodes and their grid, the conjugate scalars, the border of a conjugate entry, the 16-term tile products
// with w0, the grouped blocked back substitution with its group dispatch and LDS size, and the noise floor of the pivots.
// One definition each; every sum here runs in an order fixed by its arguments, so the callers' bits are one function's bits.
#include "posterior_device_prims.h"

namespace {

constexpr int SB = 64;                 // super-block edge
constexpr int NTHREADS = 256;
constexpr int NG = 4;                  // columns (right-hand sides, sizes) per group of the back substitution

// ((a + b) + c) + d: the one order in which four partial sums meet
__device__ __forceinline__ double sum4(const double a, const double b, const double c, const double d) { return ((a + b) + c) + d; }
__device__ __forceinline__ double sum4(const double* p) { return sum4(p[0], p[1], p[2], p[3]); }

// ------------------------------------------------------------------------------------------------
// XCD-aware mapping of a 1-D grid to (window or entry, tile) for the kernels that run SEVERAL workgroups per window.
// MI355X deals consecutive workgroup ids round-robin to its 8 XCDs, each with its own 4 MB L2.  With
// (window, tile) = (blockIdx.x, blockIdx.y) the tiles of one window ran on one XCD but thousands of workgroups
// apart, so every tile re-read the window's rows (or arena tiles) from HBM / Infinity Cache: the Gram kernel
// moved 48 GB per launch at k = 500.  Here id -> xcd = id % 8, slot = id / 8, tile = slot % NT: the NT tiles of a window
// are consecutive ON ONE XCD, whose L2 then serves the re-reads.  Two dealing orders, one grid (xcd_grid):
//   xcd_window_tile   window = 8 (slot / NT) + xcd: neighbouring windows side by side on the eight XCDs (the run)
//   xcd_entry_tile    entry = xcd ceil(e_count / 8) + slot / NT: the entries in eight contiguous runs, so that the entries of
//                     one window (its priors, shifts, lengths) follow each other on ONE XCD, whose L2 serves their reads of
//                     the window's matrices; tile -> super-tile (I, J), I <= J < NS (the sweeps' fill kernels)
// A false return is uniform per workgroup: callers return on it in front of every barrier.
__device__ __forceinline__ bool xcd_window_tile(int NT, long long G, long long& wl, int& tile) {
    const long long id = blockIdx.x;
    const long long slot = id >> 3;
    wl = 8 * (slot / NT) + (id & 7);
    tile = (int)(slot % NT);
    return wl < G;
}
__device__ __forceinline__ bool xcd_entry_tile(int NS, long long e_count, long long& e, int& I, int& J) {
    const int NT = NS * (NS + 1) / 2;
    const long long id = blockIdx.x;
    const long long slot = id >> 3;
    e = (id & 7) * ((e_count + 7) / 8) + slot / NT;
    if (e >= e_count) return false;
    pair_decode((int)(slot % NT), NS, I, J);
    return true;
}
inline dim3 xcd_grid(int NT, long long G) { return dim3((unsigned)(((G + 7) / 8) * 8 * NT)); }
inline dim3 xcd_entry_grid(int NS, long long e_count) { return xcd_grid(NS * (NS + 1) / 2, e_count); }

// ------------------------------------------------------------------------------------------------
// The conjugate scalars, in the run kernels' operation order.  hf_rows: the intraday row count m of window w.
template <class KARGS>
__device__ __forceinline__ double hf_rows(const KARGS& A, const long long w) { return (double)(A.hf_count != nullptr ? A.hf_count[w] : A.m); }
// a = n0 m/(m-1)                                                                                          (ref:333)
__device__ __forceinline__ double prior_scale(const double n0, const double mm) { return n0 * (mm / (mm - 1.0)); }
// c = 2 n0 / (g + sqrt(g^2 + 4 n0 q0)), g = n0 + k + 2 (k: the size of the system, k_s for a prefix)     (ref:415-418)
__device__ __forceinline__ double shrink_c(const double n0, const int k, const double q0) {
    const double g = n0 + k + 2;
    return (2 * n0) / (g + sqrt(g * g + 4 * n0 * q0));
}

struct EntryScal { double s, c, q0, n0; };     // ws.scal of an entry: (s, sqrt s, c, q0, n0)

// What tiled_clear_kernel leaves of an entry besides its border column, piece by piece (one thread writes the scalars) ...
__device__ __forceinline__ void write_scal(const tp_tiled_ws_t& ws, const long long e, const EntryScal& sc) {
    double* o = ws.scal + e * 8;
    o[0] = sc.s; o[1] = sqrt(sc.s); o[2] = sc.c; o[3] = sc.q0; o[4] = sc.n0;
}
// (rows >= k of the bordered matrix are never pivots: zeroed, the last diagonal block sees zero rows there)
__device__ __forceinline__ void zero_border_rows(const tp_tiled_ws_t& ws, const long long e, const int k) {
    const int KP = ws.KP;
    double* M = ws.arena + e * (long long)KP * KP;
    for (int x = threadIdx.x; x < (KP - k) * KP; x += NTHREADS) M[(long long)k * KP + x] = 0.0;
}
// ... and in one for the sweeps' border kernels: ws.scal written, the not-positive-definite flag cleared, rows >= k zeroed
__device__ __forceinline__ void close_entry(const tp_tiled_ws_t& ws, const long long e, const int k, const EntryScal& sc) {
    if (threadIdx.x == 0) { write_scal(ws, e, sc); ws.flags[e] = 0; }
    zero_border_rows(ws, e, k);
}

// v_i = the sum of row i's 64-row pieces part[((i / 64) nstride + src) 64 + i % 64], src = 0 .. nsrc-1 in this order, into
// v[i ldv], i < n; returns w0'v to every thread (wave sums, then the four wavefronts' in order).  One barrier.
__device__ __forceinline__ double pieces_dot(const double* part, const int nstride, const int nsrc, const int n,
                                             const double* w0, double* v, const long long ldv) {
    __shared__ double red[4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    double qq = 0.0;
    for (int i = tid; i < n; i += NTHREADS) {
        const double* pp = part + ((long long)(i >> 6) * nstride) * SB + (i & 63);
        double s = 0.0;
        for (int src = 0; src < nsrc; ++src) s += pp[src * SB];
        v[i * ldv] = s;
        qq = fma(w0[i], s, qq);
    }
    qq = wave_sum64(qq);
    if (lane == 0) red[wv] = qq;
    __syncthreads();
    return sum4(red);
}

// Border of a conjugate entry whose C w0 pieces (NS x NS x 64 at `part`, already scaled by a) the fill has left: v = a C w0 into
// the scratch v0, q0 = w0'v, c, and c v added to column k of the arena; n0p: where the entry's n0 lies, mm: its intraday row
// count.  Returns the entry's scalars (write_scal).
__device__ __forceinline__ EntryScal conj_border(const tp_tiled_ws_t& ws, const long long e, const int k, const double* part,
                                                 const double* w0, const double* n0p, const double mm, double* v0) {
    // k >= 1 is every launcher's guard (tp_tiled_gram_launch and the prior sweep's launcher return on k < 1): with it the
    // addresses below need no sign extension of k
    __builtin_assume(k > 0);
    const int KP = ws.KP, NS = ws.NS;
    double* M = ws.arena + e * (long long)KP * KP;
    EntryScal sc;
    sc.q0 = pieces_dot(part, NS, NS, k, w0, v0, 1);
    sc.n0 = *n0p;                               // (read behind the barrier, as the scalars are needed)
    sc.s = prior_scale(sc.n0, mm);
    sc.c = shrink_c(sc.n0, k, sc.q0);
    for (int i = threadIdx.x; i < k; i += NTHREADS) M[(long long)i * KP + k] += sc.c * v0[i];
    return sc;
}

// Quarter h of the products of a 64 x 64 tile of C (tc, super-tile (I, J)) with w0: 16 terms of row c against the columns' w0
// (wJ) and of column c against the rows' w0 (wI).  PREFIX: terms at or beyond ks are selected out, never multiplied by zero.
// The four quarters meet by sum4.
template <bool PREFIX>
__device__ __forceinline__ void tile_products16(const double (*tc)[SB + 1], const double* wI, const double* wJ, const int c, const int h,
                                                const int I, const int J, const int ks, double& sr, double& sc) {
    sr = 0.0; sc = 0.0;
#pragma unroll
    for (int i = 16 * h; i < 16 * h + 16; ++i) {
        sr = (!PREFIX || SB * J + i < ks) ? fma(tc[c][i], wJ[i], sr) : sr;
        sc = (!PREFIX || SB * I + i < ks) ? fma(tc[i][c], wI[i], sc) : sc;
    }
}

// ------------------------------------------------------------------------------------------------
// Blocked back substitution of G forward-substituted columns col0 .. col0 + G - 1 of the arena matrix M (KP x KP, upper factor
// R in rows < k) with the stored inverse diagonal blocks rinv [blk0 + Jb][64][64] (blk0: the entry's first): over block rows Jb from
// the last to 0,
//     z = y_Jb - sum_{c >= 64 (Jb+1)} R[row][c] w[c]     (16 lanes per row, 16 rows per pass, rowgroup_sum16)
//     w_Jb = R_JbJb^-1 z
// with two barriers per block row.  The solutions are left in wvec [G][KP]; zv [G][64] is scratch.  Every element of R read
// feeds G accumulators, and a column's arithmetic does not depend on which other columns share its group.
// PREFIX = false: the whole system of k for every column (ks is not read).  PREFIX = true: column g is the prefix system of
// ks[g] (increasing): block rows ceil(ks[g]/64)-1 .. 0, the dot products cut at column ks[g] and, in its last block, the
// leading ks[g] - 64 Jb rows and columns of the inverse block (the leading block of a triangular inverse is the inverse of
// the leading block) - by selects, never by a multiplication with zero.
template <int G, bool PREFIX>
__device__ __forceinline__ void back_substitute(const double* M, const int KP, const int k, const int NSB, const int col0,
                                                const double* rinv_all, const long long blk0, const int* ks, double* wvec, double* zv) {
    const int tid = threadIdx.x;
    const int srow = tid >> 4, cb = tid & 15;      // 16 lanes per row, 16 rows per pass
    int kg[G];
#pragma unroll
    for (int g = 0; g < G; ++g) kg[g] = PREFIX ? ks[g] : k;
    const int kmax = kg[G - 1];
    for (int Jb = PREFIX ? (kmax + SB - 1) / SB - 1 : NSB - 1; Jb >= 0; --Jb) {
        int np[G];                                  // rows of the block inside the column's system (<= 0: the column rests)
#pragma unroll
        for (int g = 0; g < G; ++g) np[g] = kg[g] - 64 * Jb < SB ? kg[g] - 64 * Jb : SB;
        const int npmax = np[G - 1];
        for (int ps = 0; ps < 4; ++ps) {
            const int i = 16 * ps + srow;                 // local row
            const long long gi = 64 * Jb + i;
            double s[G];
#pragma unroll
            for (int g = 0; g < G; ++g) s[g] = 0.0;
            if (i < npmax)
                for (int c = 64 * (Jb + 1) + cb; c < kmax; c += 16) {
                    const double m = M[gi * KP + c];
#pragma unroll
                    for (int g = 0; g < G; ++g) s[g] = (!PREFIX || c < kg[g]) ? fma(m, wvec[g * KP + c], s[g]) : s[g];
                }
#pragma unroll
            for (int g = 0; g < G; ++g) s[g] = rowgroup_sum16(s[g]);
            if (cb == 0) {
#pragma unroll
                for (int g = 0; g < G; ++g) zv[g * SB + i] = (i < np[PREFIX ? g : G - 1]) ? M[gi * KP + col0 + g] - s[g] : 0.0;
            }
        }
        __syncthreads();
        const double* rinv = rinv_all + (blk0 + Jb) * (long long)(SB * SB);
        for (int ps = 0; ps < 4; ++ps) {
            const int i = 16 * ps + srow;
            double s[G];
#pragma unroll
            for (int g = 0; g < G; ++g) s[g] = 0.0;
            if (!PREFIX || i < npmax)
                for (int c = cb; c < SB; c += 16) {
                    const double rv = rinv[i * SB + c];
#pragma unroll
                    for (int g = 0; g < G; ++g) s[g] = (!PREFIX || c < np[g]) ? fma(rv, zv[g * SB + c], s[g]) : s[g];
                }
#pragma unroll
            for (int g = 0; g < G; ++g) s[g] = rowgroup_sum16(s[g]);
            if (cb == 0 && (PREFIX || i < npmax)) {
#pragma unroll
                for (int g = 0; g < G; ++g)
                    if (!PREFIX || i < np[g]) wvec[g * KP + 64 * Jb + i] = s[g];
            }
        }
        __syncthreads();
    }
}

// f(ic<G>, g0) for the n columns in groups of NG: g0 = 0, NG, ..., G = the group's count.  Uniform per workgroup, so every
// thread reaches every barrier of every group.
template <class F>
__device__ __forceinline__ void for_each_group(const int n, F&& f) {
    for (int g0 = 0; g0 < n; g0 += NG) {
        const int g = n - g0 < NG ? n - g0 : NG;
        if (g == 4) f(ic<4>{}, g0);
        else if (g == 3) f(ic<3>{}, g0);
        else if (g == 2) f(ic<2>{}, g0);
        else f(ic<1>{}, g0);
    }
}

// Dynamic LDS of a grouped solve kernel over n columns, wvec [min(n, NG)][KP] | zv [NG][64], allowed for `kernel` up to the
// largest geometry (KP <= 2048); hipErrorInvalidValue beyond it.
template <class KERNEL>
inline hipError_t group_solve_lds(std::atomic<unsigned long long>& done_mask, KERNEL kernel, const int n, const int KP, size_t* smem) {
    const int max_lds = (int)(sizeof(double) * (size_t)(NG * SB * 32 + NG * SB));
    *smem = sizeof(double) * ((size_t)(n < NG ? n : NG) * KP + NG * SB);
    if (*smem > (size_t)max_lds) return hipErrorInvalidValue;
    return tp_allow_dynamic_lds(done_mask, kernel, max_lds);
}

// Noise floor of the pivots of a system of n: true when some i < n has d_i <= n 2^-52 M_ii (the floor of the LDS prior sweep),
// d_i = 1 / (R^-1)_ii^2 from the diagonals of the entry's inverse diagonal blocks rinv0, M_ii = mii_of(i).  An exactly
// repeated column has a pivot that is zero in exact arithmetic and of either sign in floating point; "not > 0" alone lets the
// positive ones through as finite garbage with status OK.  A NaN fails the comparison too.  Per thread: the caller gathers.
template <class F>
__device__ __forceinline__ bool low_pivot(const double* rinv0, const int n, F&& mii_of) {
    const double rel = (double)n * 0x1p-52;
    bool low = false;
    for (int i = threadIdx.x; i < n; i += NTHREADS) {
        const double ri = rinv0[(long long)(i >> 6) * (SB * SB) + (i & 63) * (SB + 1)];
        if (!(1.0 > rel * mii_of(i) * (ri * ri))) low = true;
    }
    return low;
}

}  // namespace
