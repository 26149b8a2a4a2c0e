// posterior_grid_sweep_tiled.h - internal interface between the sweeps of the C-ABI (tangency_sweep.cpp) and the kernels of the
// grid sweep on the large-k tiled path (posterior_grid_sweep_tiled.hip, tp_batch_grid_sweep_tiled).  The Gram stages are the
// tiled window sweep's, unchanged: the batch's tiled Gram stage over the intraday rows (C), tp_tiled_window_gram_launch and
// tp_window_delta_launch (posterior_window_sweep.h).
#pragma once
#include "posterior_kernels.h"

// Arena entry e of a group is the (window, prior, length) with the flat index e_first + e = (w P + p) L + l.  The workspace is the
// solve sweep's (tp_solve_sweep_tiled_geometry with R = S: KP from k + S); it uses ws.arena, ws.rinv and ws.flags.  C / T hold the
// matrices of the windows [wc_first, ..) of the sub-range, cv / cq the prior products of its (window, prior) pairs, mdiag the
// diagonals of one group's entries; every other array is indexed by the numbers in the batch.
//   conjugate (C != nullptr): C = Y'Y - (Y'1)(Y'1)'/m (symmetric, full storage); n0 and w0 are the caller's priors.
//   Jeffreys  (C == nullptr): P = 1, n0 = w0 = cv = cq = nullptr; center_rows as tp_kargs_t (0: / N[l], 1: / rows[w][l], 2: no term).
struct tp_grid_sweep_tiled_kargs_t {
    const double* C;            // [chunk x k x k], or nullptr: Jeffreys
    const double* T;            // [chunk x L x k x k], column >= row valid
    const double* t;            // [W x L x k]
    const double* dv;           // [W x L x k], or nullptr: no delta
    const double* ds;           // [W x L x 2], or nullptr
    const double* n0;           // [W x P x L]
    const double* w0;           // [W x P x S x k]; entries at or beyond sizes[s] are never read
    const int* hf_count;        // optional [W]: intraday rows of the window (else m)
    const int* rows;            // [W x L]
    const int* N;               // [L] (device memory)
    const int* sizes;           // [S], strictly increasing within [1, k] (device memory)
    double* cv;                 // [chunk x P x S x k]: v_s = C[:k_s,:k_s] w0_wps[:k_s] on rows < k_s (the rest is never read)
    double* cq;                 // [chunk x P x S]: w0_wps'v_s
    double* mdiag;              // [entries of one group x k]: the diagonal the fill writes
    double* weights;            // [W x P x L x S x k]; entries at or beyond sizes[s] are written as 0
    int* status;                // [W x P x L x S]
    double* aux;                // [W x P x L x S x 8]: n0, n1, c, q0, q1, n1 - q1, 0, 0 (Jeffreys: 0, 0, 0, 0, q1, 0, 0, 0)
    long long wc_first;         // first window of the sub-range
    long long wp_first, wp_count;   // the prior products' launch: the (window, prior) pairs [wp_first, wp_first + wp_count)
    long long e_first, e_count; // e_count <= the workspace's capacity
    int k, P, L, S, m, center_rows;
    double gamma;
};
// v_s and w0'v_s for the pairs of a sub-range: once per (window, prior), whatever L and n0 are (conjugate)
hipError_t tp_grid_sweep_tiled_cw_launch(const tp_grid_sweep_tiled_kargs_t& a, hipStream_t stream);
// fills the entries: the matrix of length l inside k x k, size s's right-hand side on rows < k_s of column k + s, zero elsewhere,
// the flag cleared, the diagonal into mdiag, c_s and q0_s into the aux rows; tp_tiled_block_steps_launch factorises them; the
// solve back-substitutes every size over its prefix and writes the weights, statuses and aux rows to their slots
hipError_t tp_grid_sweep_tiled_fill_launch(const tp_grid_sweep_tiled_kargs_t& a, const tp_tiled_ws_t& ws, hipStream_t stream);
hipError_t tp_grid_sweep_tiled_solve_launch(const tp_grid_sweep_tiled_kargs_t& a, const tp_tiled_ws_t& ws, hipStream_t stream);
