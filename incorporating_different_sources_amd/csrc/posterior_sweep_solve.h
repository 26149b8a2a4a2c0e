#pragma once
// posterior_sweep_solve.h - the LDS factorisation and back substitution the sweep kernels share (posterior_sweep.hip: many
// shifts and right-hand sides; posterior_prior_sweep.hip: many conjugate priors; posterior_size_sweep.hip: nested universes,
// solved over prefixes of one factorisation).  One 256-thread workgroup owns one
// matrix: its lower triangle in PACKED storage, column by column, with R right-hand sides riding along as R extra rows,
//
//     column c holds rows i = c .. k + R - 1 at  off(c) + (i - c),   off(c) = c (k + R) - c (c - 1) / 2 .
//
// The order of operations depends on k and R only.  Workgroup barriers only, each reached by every thread whatever the
// pivots are; nothing spins.
#include "posterior_device_prims.h"

namespace {

constexpr int SWEEP_THREADS = 256;
constexpr int SWEEP_TX = 32;            // lanes along a column
constexpr int SWEEP_TY = SWEEP_THREADS / SWEEP_TX;
constexpr int SWEEP_XREGS = 3;          // solution registers per lane: k <= 64 * 3
constexpr int SWEEP_MAX_K = 143;        // 16 x 9 - 1: the one-wave kernels' range; 98.3 KiB of LDS at R = 16

__device__ __forceinline__ int sweep_off(int c, int H) { return c * H - (c * (c - 1)) / 2; }

// Right-looking, square-root-free Cholesky M = L D L' kept UNSCALED (column j holds l_ij d_j), in place.  Step j reads the
// pivot d_j = A[j][j] and subtracts A[i][j] A[c][j] / d_j from every element (i, c), j < c < k, c <= i < H.  Nothing of column
// j is rewritten in step j, so ONE workgroup barrier per column is all the synchronisation there is.  The extra rows come out
// as the forward substitution: row k + r ends as y~_j = (L^-1 b_r)_j = d_j (L' x_r)_j.  Returns whether a pivot was <= its
// floor - floor[j], or 0 without one - (the same answer in every thread; a NaN pivot is not "<=": it ends as a non-finite
// solution).  The image must be complete and a barrier passed before the call; the call ends behind a barrier.
__device__ __forceinline__ bool sweep_ldl_factor(double* lds, int k, int H, int tid, const double* floor = nullptr) {
    const int tx = tid & (SWEEP_TX - 1), ty = tid / SWEEP_TX;
    bool notpd = false;
    for (int j = 0; j < k; ++j) {
        const double* cj = lds + sweep_off(j, H) - j;          // cj[i] = A[i][j]
        const double dj = cj[j];
        if (dj <= (floor != nullptr ? floor[j] : 0.0)) notpd = true;
        const double inv = 1.0 / dj;
        for (int c = j + 1 + ty; c < k; c += SWEEP_TY) {
            const double m = cj[c] * inv;
            double* cc = lds + sweep_off(c, H) - c;
            for (int i = c + tx; i < H; i += SWEEP_TX) cc[i] -= cj[i] * m;
        }
        __syncthreads();
    }
    return notpd;
}

// Back substitution of right-hand side r by ONE wavefront, no workgroup barrier.  The solution stays in registers - lane l
// owns x_i for i = l, l + 64, l + 128 - and step j = k-1 .. 0 is a dot product of the contiguous column j with those
// registers, a wave all-reduce (fixed butterfly order) and x_j = (y~_j - sum_{i > j} A[i][j] x_i) / d_j.
__device__ __forceinline__ void sweep_back_substitute(const double* lds, int k, int H, int r, int lane, double (&x)[SWEEP_XREGS]) {
#pragma unroll
    for (int q = 0; q < SWEEP_XREGS; ++q) x[q] = 0.0;
    for (int j = k - 1; j >= 0; --j) {
        const double* cj = lds + sweep_off(j, H) - j;
        double part = 0.0;
#pragma unroll
        for (int q = 0; q < SWEEP_XREGS; ++q) {
            const int i = lane + 64 * q;
            if (i > j && i < k) part += cj[i] * x[q];
        }
        const double xj = (cj[k + r] - wave_sum64(part)) / cj[j];
#pragma unroll
        for (int q = 0; q < SWEEP_XREGS; ++q)
            if (lane + 64 * q == j) x[q] = xj;
    }
}

// The same back substitution over the leading kp x kp block (posterior_size_sweep.hip): step j = kp-1 .. 0, the dot product
// over j < i < kp, the right-hand side still in row k + r.  The leading block of the factor is the factor of the leading
// block, and entry j of a forward-substituted row depends on columns <= j only, so this solves the first kp columns' own
// system.  With kp = k it is sweep_back_substitute, operation for operation.
__device__ __forceinline__ void sweep_back_substitute_prefix(const double* lds, int k, int H, int kp, int r, int lane,
                                                             double (&x)[SWEEP_XREGS]) {
#pragma unroll
    for (int q = 0; q < SWEEP_XREGS; ++q) x[q] = 0.0;
    for (int j = kp - 1; j >= 0; --j) {
        const double* cj = lds + sweep_off(j, H) - j;
        double part = 0.0;
#pragma unroll
        for (int q = 0; q < SWEEP_XREGS; ++q) {
            const int i = lane + 64 * q;
            if (i > j && i < kp) part += cj[i] * x[q];
        }
        const double xj = (cj[k + r] - wave_sum64(part)) / cj[j];
#pragma unroll
        for (int q = 0; q < SWEEP_XREGS; ++q)
            if (lane + 64 * q == j) x[q] = xj;
    }
}

}  // namespace
