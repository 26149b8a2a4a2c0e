// posterior_grid_sweep.h - internal interface between the sweeps of the C-ABI (tangency_sweep.cpp) and the kernel of the grid
// sweep (posterior_grid_sweep.hip).  The Gram stages are the window sweep's, unchanged: tp_window_gram_launch and
// tp_window_delta_launch (posterior_window_sweep.h).
#pragma once
#include "posterior_kernels.h"

// grid sweep (tp_batch_grid_sweep): one workgroup per (window, prior, length) of the windows [w_first, w_first + w_count), whose
// C and snapshots lie in the workspaces (window w_first first); S nested universes - the first sizes[s] columns - per
// workgroup from ONE factorisation at k.  All other arrays are indexed by the window's number in the batch.
//   conjugate (C != nullptr): n0 and w0 are the caller's priors.
//   Jeffreys  (C == nullptr): P = 1, n0 = w0 = nullptr; center_rows as tp_kargs_t (0: / N[l], 1: / rows[w][l], 2: no term).
struct tp_grid_sweep_kargs_t {
    const double* C;            // [w_count x k x k], or nullptr: Jeffreys
    const double* T;            // [w_count x L x k x k]
    const double* t;            // [W x L x k]
    const double* dv;           // [W x L x k], or nullptr: no delta
    const double* ds;           // [W x L x 2], or nullptr
    const double* n0;           // [W x P x L]
    const double* w0;           // [W x P x S x k]; entries at or beyond sizes[s] are never read
    const int* hf_count;        // optional [W]: intraday rows of the window (else m)
    const int* rows;            // [W x L]
    const int* N;               // [L] (device memory)
    const int* sizes;           // [S], strictly increasing within [1, k] (device memory)
    double* weights;            // [W x P x L x S x k]; entries at or beyond sizes[s] are written as 0
    int* status;                // [W x P x L x S]
    double* aux;                // [W x P x L x S x 8]: n0, n1, c, q0, q1, n1 - q1, 0, 0 (Jeffreys: 0, 0, 0, 0, q1, 0, 0, 0)
    long long w_first, w_count;
    int k, P, L, S, m, center_rows;
    double gamma;
};
size_t tp_grid_sweep_lds_bytes(int k, int S, bool conjugate);
hipError_t tp_grid_sweep_launch(const tp_grid_sweep_kargs_t& a, hipStream_t stream);
