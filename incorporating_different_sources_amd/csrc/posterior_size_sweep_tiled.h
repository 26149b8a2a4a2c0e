// posterior_size_sweep_tiled.h - internal interface between the sweeps of the C-ABI (tangency_sweep.cpp) and the kernels of the
// size sweep on the large-k tiled path (posterior_size_sweep_tiled.hip, tp_batch_size_sweep_tiled).
#pragma once
#include "posterior_kernels.h"

// Arena entry e of a group is the (window, prior) pair with the flat index e_first + e = w P + p.  The workspace is the solve
// sweep's (tp_solve_sweep_tiled_geometry with R = S: KP from k + S); it uses ws.arena, ws.rinv, ws.flags and, conjugate,
// ws.part [entries x S x NSB x NSB x 64]: the pieces of the truncated products C[:k_s,:k_s] w0_s.  C / T hold the matrices of
// the windows [wc_first, ..) of the sub-range (symmetric, full storage); every other array is indexed by the numbers in the batch.
//   conjugate (C != nullptr): C = Y'Y - (Y'1)(Y'1)'/m, T = X'X, t = X'1; n0 and w0 are the caller's priors.
//   Jeffreys  (C == nullptr): T holds M as the batch's Gram stage keeps it, t its right-hand side; P = 1, n0 = w0 = nullptr.
struct tp_size_sweep_tiled_kargs_t {
    const double* C;            // [windows of the sub-range x k x k], or nullptr: Jeffreys
    const double* T;            // [windows of the sub-range x k x k]
    const double* t;            // [W x k]
    const double* n0;           // [W x P]
    const double* w0;           // [W x P x S x k]; entries at or beyond sizes[s] are never read
    const int* hf_count;        // optional [W]: intraday rows of the window (else m)
    const int* sizes;           // [S], strictly increasing within [1, k] (device memory)
    double* weights;            // [W x P x S x k]; entries at or beyond sizes[s] are written as 0
    int* status;                // [W x P x S]
    double* aux;                // [W x P x S x 8]: n0, n1, c, q0, q1, n1 - q1, 0, 0 (Jeffreys: 0, 0, 0, 0, q1, 0, 0, 0)
    long long e_first, e_count; // e_count <= the workspace's capacity
    long long wc_first;         // first window of the sub-range
    int k, P, S, N, m;
    double gamma;
};
// doubles of ws.part per arena entry (conjugate)
size_t tp_size_sweep_tiled_part_doubles(int k, int S);
// fills the entries: the matrix inside k x k, size s's right-hand side on rows < k_s of column k + s, zero elsewhere, the flag
// cleared; tp_tiled_block_steps_launch factorises them; the solve back-substitutes every size over its prefix and writes the
// weights, statuses and aux rows
hipError_t tp_size_sweep_tiled_fill_launch(const tp_size_sweep_tiled_kargs_t& a, const tp_tiled_ws_t& ws, hipStream_t stream);
hipError_t tp_size_sweep_tiled_solve_launch(const tp_size_sweep_tiled_kargs_t& a, const tp_tiled_ws_t& ws, hipStream_t stream);
