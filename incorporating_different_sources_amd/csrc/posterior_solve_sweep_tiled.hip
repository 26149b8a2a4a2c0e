// posterior_solve_sweep_tiled.hip - solve sweep above the LDS solve core (tp_batch_solve_sweep_tiled, k > tp_sweep_max_assets()):
// many shifts (d, e) and R right-hand sides per window from ONE Gram pass, factorised by the large-k tiled pipeline.
//
// The Gram stage of the tiled path (tp_tiled_gram_launch, steered by its arguments: tangency_api.cpp) has stored, per window of
// the sub-range, M_w (S1 or J: k x k, symmetric, full storage) and the window's own right-hand side.  An ARENA ENTRY is one
// (window, shift) pair in a workspace of the SWEEP's geometry, KP = 64 ceil((k + R)/64), NS = KP/64, NSB = ceil(k/64): columns
// k .. k+R-1 of the arena hold the R right-hand sides.  The block steps of the tiled factorisation (tp_tiled_block_steps_launch)
// take their geometry from the workspace and carry every column >= k of a pivot block row along, so all R columns leave the
// factorisation forward-substituted (R^-T rhs); rows >= k are zero and never pivots.
//
//   solve_sweep_tiled_fill_kernel     one workgroup per (entry, super-tile (I, J), I <= J): M_w + e (+ d on the diagonal)
//                                     inside k x k, right-hand side r into column k + r, zero elsewhere; the entry's flag cleared
//   solve_sweep_tiled_solve_kernel    one workgroup per entry: blocked back substitution (tiled_solve_kernel's scheme) of the R
//                                     columns in groups of up to 4 - the solution image of a group is at most 64 KiB of LDS and
//                                     every element of R read feeds up to 4 accumulators - x / gamma and the status
//
// Plain C++, workgroup barriers only, each reached by every thread of its workgroup.  A (window, shift) result depends on the
// window's M_w, on its own shift and right-hand sides and on k alone: every sum below runs in an order fixed by k, and a
// column's arithmetic does not depend on which other columns share its group.
#include "posterior_device_prims.h"
#include "posterior_solve_sweep_tiled.h"

namespace {

constexpr int SB = 64;
constexpr int NTHREADS = 256;
constexpr int NG = 4;                          // right-hand sides per group of the back substitution

__global__ void __launch_bounds__(NTHREADS) solve_sweep_tiled_fill_kernel(const tp_solve_sweep_tiled_kargs_t A, const tp_tiled_ws_t ws) {
    const int tid = threadIdx.x;
    const int k = A.k, KP = ws.KP, NS = ws.NS;
    const int NT = NS * (NS + 1) / 2;
    // The tiled path's grid decode (workgroup id -> XCD = id % 8, slot = id / 8; tiles of an entry consecutive on one XCD),
    // with the entries dealt to the XCDs in eight contiguous runs: the S entries of a window follow each other on ONE XCD,
    // whose L2 then serves their reads of the window's M_w.
    const long long id = blockIdx.x;
    const long long slot = id >> 3;
    const long long per_xcd = (A.e_count + 7) / 8;
    const long long e = (id & 7) * per_xcd + slot / NT;
    if (e >= A.e_count) return;                 // (uniform per workgroup; the kernel has no barrier)
    const int tile = (int)(slot % NT);
    int I, J;
    pair_decode(tile, NS, I, J);
    const long long f = A.e_first + e;         // flat (window, shift) index
    const long long w = f / A.S;
    const double* __restrict__ P = A.post + (w - A.wc_first) * (long long)k * k;
    const double sh_d = A.shift ? A.shift[2 * f] : 0.0;
    const double sh_e = A.shift ? A.shift[2 * f + 1] : 0.0;
    double* M = ws.arena + e * (long long)KP * KP;
    const int c = tid & (SB - 1), q = tid >> 6;
    const int gj = SB * J + c;                  // < KP
    // column gj >= k: right-hand side r = gj - k (slot 0 is the window's own one when there is a default)
    const int r = gj - k;
    const double* __restrict__ col = nullptr;
    if (r >= 0 && r < A.R) {
        const int nd = A.default_rhs != nullptr ? 1 : 0;
        col = r < nd ? A.default_rhs + w * k : A.rhs + (w * A.n_rhs + (r - nd)) * (long long)k;
    }
    for (int rr = q; rr < SB; rr += NTHREADS / SB) {
        const int gi = SB * I + rr;             // < KP
        double v = 0.0;                         // rows >= k, columns >= k + R
        if (gi < k) {
            if (gj < k) v = P[(long long)gi * k + gj] + (sh_e + (gi == gj ? sh_d : 0.0));
            else if (col != nullptr) v = col[gi];
        }
        M[(long long)gi * KP + gj] = v;
    }
    if (tile == 0 && tid == 0) ws.flags[e] = 0;
}

// back substitution of columns k + g0 .. k + g0 + G - 1 of one entry; wvec [G][KP] | zv [G][64]
template <int G>
__device__ __forceinline__ bool solve_group(const tp_solve_sweep_tiled_kargs_t& A, const tp_tiled_ws_t& ws, const long long e,
                                            const int g0, double* wvec, double* zv) {
    const int tid = threadIdx.x;
    const int k = A.k, KP = ws.KP, NSB = ws.NSB;
    const double* M = ws.arena + e * (long long)KP * KP;
    const int srow = tid >> 4, cb = tid & 15;      // 16 lanes per row, 16 rows per pass
    for (int Jb = NSB - 1; Jb >= 0; --Jb) {
        const int npiv = (k - 64 * Jb < SB) ? (k - 64 * Jb) : SB;
        // z = y_Jb - sum_{c >= 64 (Jb+1)} R[row][c] w[c], y = the forward-substituted columns
        for (int ps = 0; ps < 4; ++ps) {
            const int i = 16 * ps + srow;                 // local row
            const long long gi = 64 * Jb + i;
            double s[G];
#pragma unroll
            for (int g = 0; g < G; ++g) s[g] = 0.0;
            if (i < npiv)
                for (int c = 64 * (Jb + 1) + cb; c < k; c += 16) {
                    const double m = M[gi * KP + c];
#pragma unroll
                    for (int g = 0; g < G; ++g) s[g] = fma(m, wvec[g * KP + c], s[g]);
                }
#pragma unroll
            for (int g = 0; g < G; ++g) s[g] = rowgroup_sum16(s[g]);
            if (cb == 0) {
#pragma unroll
                for (int g = 0; g < G; ++g) zv[g * SB + i] = (i < npiv) ? M[gi * KP + k + g0 + g] - s[g] : 0.0;
            }
        }
        __syncthreads();
        // w_Jb = R_jj^-1 z
        const double* rinv = ws.rinv + (e * NSB + Jb) * (long long)(SB * SB);
        for (int ps = 0; ps < 4; ++ps) {
            const int i = 16 * ps + srow;
            double s[G];
#pragma unroll
            for (int g = 0; g < G; ++g) s[g] = 0.0;
            for (int c = cb; c < SB; c += 16) {
                const double rv = rinv[i * SB + c];
#pragma unroll
                for (int g = 0; g < G; ++g) s[g] = fma(rv, zv[g * SB + c], s[g]);
            }
#pragma unroll
            for (int g = 0; g < G; ++g) s[g] = rowgroup_sum16(s[g]);
            if (cb == 0 && i < npiv) {
#pragma unroll
                for (int g = 0; g < G; ++g) wvec[g * KP + 64 * Jb + i] = s[g];
            }
        }
        __syncthreads();
    }
    const long long f = A.e_first + e;
    bool bad = false;
#pragma unroll
    for (int g = 0; g < G; ++g) {
        double* x = A.x + (f * A.R + g0 + g) * (long long)k;
        for (int i = tid; i < k; i += NTHREADS) {
            const double out = 1.0 / A.gamma * wvec[g * KP + i];
            x[i] = out;
            if (!isfinite(out)) bad = true;
        }
    }
    __syncthreads();                               // the next group overwrites wvec
    return bad;
}

__global__ void __launch_bounds__(NTHREADS) solve_sweep_tiled_solve_kernel(const tp_solve_sweep_tiled_kargs_t A, const tp_tiled_ws_t ws) {
    extern __shared__ __attribute__((aligned(16))) double sm[];     // wvec [min(R, NG)][KP] | zv [NG][64]
    __shared__ int anybad, anylow;
    const long long e = blockIdx.x;
    const int R = A.R;
    double* wvec = sm;
    double* zv = sm + (R < NG ? R : NG) * ws.KP;
    if (threadIdx.x == 0) { anybad = 0; anylow = 0; }
    __syncthreads();
    bool bad = false;
    for (int g0 = 0; g0 < R; g0 += NG) {           // (uniform: every thread reaches every barrier of every group)
        const int g = R - g0 < NG ? R - g0 : NG;
        if (g == 4) bad |= solve_group<4>(A, ws, e, g0, wvec, zv);
        else if (g == 3) bad |= solve_group<3>(A, ws, e, g0, wvec, zv);
        else if (g == 2) bad |= solve_group<2>(A, ws, e, g0, wvec, zv);
        else bad |= solve_group<1>(A, ws, e, g0, wvec, zv);
    }
    if (bad) anybad = 1;
    // A pivot at the rounding noise of its own diagonal element is not positive definite either: d_i <= k 2^-52 M_ii, the floor
    // of the LDS prior sweep.  An exactly repeated column has a pivot that is zero in exact arithmetic and of either sign in
    // floating point; "not > 0" alone let the positive ones through as finite garbage with status OK.  d_i = 1 / (R^-1)_ii^2
    // from the inverse diagonal blocks the back substitution has just used, M_ii from the kept matrix and the entry's shift.
    {
        const int k = A.k;
        const long long f = A.e_first + e;
        const double* __restrict__ P = A.post + (f / A.S - A.wc_first) * (long long)k * k;
        const double sh = A.shift ? A.shift[2 * f] + A.shift[2 * f + 1] : 0.0;
        const double* rinv = ws.rinv + e * ws.NSB * (long long)(SB * SB);
        bool low = false;
        for (int i = threadIdx.x; i < k; i += NTHREADS) {
            const double ri = rinv[(long long)(i >> 6) * (SB * SB) + (i & 63) * (SB + 1)];
            if (!(1.0 > (k * 0x1p-52) * (P[(long long)i * k + i] + sh) * (ri * ri))) low = true;     // (a NaN ends here too)
        }
        if (low) anylow = 1;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int st = TP_KSTATUS_OK;
        if (ws.flags[e] || anylow) st = TP_KSTATUS_NOT_PD;
        else if (anybad) st = TP_KSTATUS_NONFINITE;
        A.status[A.e_first + e] = st;
    }
}

}  // namespace

void tp_solve_sweep_tiled_geometry(int k, int R, int* KP, int* NS, int* NSB) {
    const int ns = (k + R + SB - 1) / SB;
    *NS = ns; *KP = ns * SB; *NSB = (k + SB - 1) / SB;
}

hipError_t tp_solve_sweep_tiled_fill_launch(const tp_solve_sweep_tiled_kargs_t& a, const tp_tiled_ws_t& ws, hipStream_t stream) {
    if (a.k < 1 || a.S < 1 || a.R < 1 || a.R > TP_SWEEP_KMAX_RHS || a.e_count < 1 || a.e_count > 65535 || a.k + a.R > ws.KP ||
        ws.KP != SB * ws.NS || ws.NSB != (a.k + SB - 1) / SB || (a.n_rhs > 0 && a.rhs == nullptr) ||
        a.R != (a.default_rhs != nullptr ? 1 : 0) + a.n_rhs)
        return hipErrorInvalidValue;
    const long long NT = (long long)ws.NS * (ws.NS + 1) / 2;
    const long long grid = ((a.e_count + 7) / 8) * 8 * NT;
    hipLaunchKernelGGL(solve_sweep_tiled_fill_kernel, dim3((unsigned)grid), dim3(NTHREADS), 0, stream, a, ws);
    return hipGetLastError();
}

hipError_t tp_solve_sweep_tiled_solve_launch(const tp_solve_sweep_tiled_kargs_t& a, const tp_tiled_ws_t& ws, hipStream_t stream) {
    if (a.k < 1 || a.R < 1 || a.R > TP_SWEEP_KMAX_RHS || a.e_count < 1 || a.e_count > 65535 || a.k + a.R > ws.KP)
        return hipErrorInvalidValue;
    const int max_lds = (int)(sizeof(double) * (size_t)(NG * SB * 32 + NG * SB));       // KP <= 2048
    static std::atomic<unsigned long long> attr_done{0};      // one bit per device (tp_allow_dynamic_lds)
    { hipError_t e = tp_allow_dynamic_lds(attr_done, solve_sweep_tiled_solve_kernel, max_lds); if (e != hipSuccess) return e; }
    const size_t smem = sizeof(double) * ((size_t)(a.R < NG ? a.R : NG) * ws.KP + NG * SB);
    if (smem > (size_t)max_lds) return hipErrorInvalidValue;
    hipLaunchKernelGGL(solve_sweep_tiled_solve_kernel, dim3((unsigned)a.e_count), dim3(NTHREADS), smem, stream, a, ws);
    return hipGetLastError();
}
