// posterior_solve_sweep_tiled.h - internal interface between the sweeps of the C-ABI (tangency_sweep.cpp) and the two kernels of
// the solve sweep on the large-k tiled path (posterior_solve_sweep_tiled.hip, tp_batch_solve_sweep_tiled).
#pragma once
#include "posterior_kernels.h"

// Arena entry e of a group is the (window, shift) pair with the flat index e_first + e = w S + s.  The workspace is the
// SWEEP's own, with the sweep's geometry (tp_solve_sweep_tiled_geometry: KP from k + R); it uses ws.arena, ws.rinv and
// ws.flags only.  `post` holds M_w of the windows [wc_first, ..) of the sub-range (symmetric, full storage); every other
// array is indexed by the numbers in the batch.
struct tp_solve_sweep_tiled_kargs_t {
    const double* post;         // [windows of the sub-range x k x k]
    const double* default_rhs;  // optional [W x k]: slot r = 0 (the window's own right-hand side)
    const double* rhs;          // optional [W x n_rhs x k]: the caller's columns, behind the default
    const double* shift;        // optional [W x S x 2] = (d, e): adds d I + e 1 1'
    double* x;                  // [W x S x R x k]
    int* status;                // [W x S]
    long long e_first, e_count; // e_count <= the workspace's capacity
    long long wc_first;         // first window of the sub-range
    int k, S, R, n_rhs;         // R = (default_rhs ? 1 : 0) + n_rhs
    double gamma;
};
// KP = 64 ceil((k + R)/64), NS = KP/64, NSB = ceil(k/64): columns k .. k+R-1 hold the right-hand sides
void tp_solve_sweep_tiled_geometry(int k, int R, int* KP, int* NS, int* NSB);
// fills the entries (matrix, right-hand sides, zero border, flags); tp_tiled_block_steps_launch factorises them; the solve
// back-substitutes the R columns and writes x / gamma and the statuses
hipError_t tp_solve_sweep_tiled_fill_launch(const tp_solve_sweep_tiled_kargs_t& a, const tp_tiled_ws_t& ws, hipStream_t stream);
hipError_t tp_solve_sweep_tiled_solve_launch(const tp_solve_sweep_tiled_kargs_t& a, const tp_tiled_ws_t& ws, hipStream_t stream);
