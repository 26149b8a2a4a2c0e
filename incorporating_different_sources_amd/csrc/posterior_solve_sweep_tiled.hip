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
//   solve_sweep_tiled_solve_kernel    one workgroup per entry: blocked back substitution (back_substitute, as tiled_solve_kernel)
//                                     of the R columns in groups of up to 4 - the solution image of a group is at most 64 KiB
//                                     of LDS - x / gamma and the status
//
// The grid decode, the back substitution with its group dispatch and LDS size, and the pivot floor are
// posterior_tiled_sweep_prims.h's.
//
// Plain C++, workgroup barriers only, each reached by every thread of its workgroup.  A (window, shift) result depends on the
// window's M_w, on its own shift and right-hand sides and on k alone: every sum below runs in an order fixed by k, and a
// column's arithmetic does not depend on which other columns share its group.
#include "posterior_tiled_sweep_prims.h"
#include "posterior_solve_sweep_tiled.h"

namespace {

__global__ void __launch_bounds__(NTHREADS) solve_sweep_tiled_fill_kernel(const tp_solve_sweep_tiled_kargs_t A, const tp_tiled_ws_t ws) {
    const int tid = threadIdx.x;
    const int k = A.k, KP = ws.KP, NS = ws.NS;
    long long e;
    int I, J;
    if (!xcd_entry_tile(NS, A.e_count, e, I, J)) return;
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
    if (J == 0 && tid == 0) ws.flags[e] = 0;       // (super-tile (0, 0))
}

// back substitution of columns k + g0 .. k + g0 + G - 1 of one entry and x = w / gamma; wvec [G][KP] | zv [G][64]
template <int G>
__device__ __forceinline__ bool solve_group(const tp_solve_sweep_tiled_kargs_t& A, const tp_tiled_ws_t& ws, const long long e,
                                            const int g0, double* wvec, double* zv) {
    const int tid = threadIdx.x;
    const int k = A.k, KP = ws.KP;
    back_substitute<G, false>(ws.arena + e * (long long)KP * KP, KP, k, ws.NSB, k + g0, ws.rinv, e * ws.NSB, nullptr, wvec, zv);
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
    for_each_group(R, [&](auto G, const int g0) { bad |= solve_group<decltype(G)::value>(A, ws, e, g0, wvec, zv); });
    if (bad) anybad = 1;
    // the pivots' noise floor (low_pivot), M_ii from the kept matrix and the entry's shift
    {
        const int k = A.k;
        const long long f = A.e_first + e;
        const double* __restrict__ P = A.post + (f / A.S - A.wc_first) * (long long)k * k;
        const double sh = A.shift ? A.shift[2 * f] + A.shift[2 * f + 1] : 0.0;
        if (low_pivot(ws.rinv + e * ws.NSB * (long long)(SB * SB), k, [&](const int i) { return P[(long long)i * k + i] + sh; })) anylow = 1;
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
    hipLaunchKernelGGL(solve_sweep_tiled_fill_kernel, xcd_entry_grid(ws.NS, a.e_count), dim3(NTHREADS), 0, stream, a, ws);
    return hipGetLastError();
}

hipError_t tp_solve_sweep_tiled_solve_launch(const tp_solve_sweep_tiled_kargs_t& a, const tp_tiled_ws_t& ws, hipStream_t stream) {
    if (a.k < 1 || a.R < 1 || a.R > TP_SWEEP_KMAX_RHS || a.e_count < 1 || a.e_count > 65535 || a.k + a.R > ws.KP)
        return hipErrorInvalidValue;
    static std::atomic<unsigned long long> attr_done{0};      // one bit per device (tp_allow_dynamic_lds)
    size_t smem;
    { hipError_t e = group_solve_lds(attr_done, solve_sweep_tiled_solve_kernel, a.R, ws.KP, &smem); if (e != hipSuccess) return e; }
    hipLaunchKernelGGL(solve_sweep_tiled_solve_kernel, dim3((unsigned)a.e_count), dim3(NTHREADS), smem, stream, a, ws);
    return hipGetLastError();
}
