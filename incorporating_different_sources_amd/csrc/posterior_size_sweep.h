// posterior_size_sweep.h - internal interface between the sweeps of the C-ABI (tangency_sweep.cpp) and the kernel of the size
// sweep (posterior_size_sweep.hip).  The Gram passes are the existing ones: tp_gram_launch (posterior_prior_sweep.h) for a
// conjugate batch, the batch's own run kernel with its kept-matrix and kept-right-hand-side stores for a Jeffreys batch.
#pragma once
#include "posterior_kernels.h"

// size sweep (tp_batch_size_sweep): one workgroup per (window, prior) of the windows [w_first, w_first + w_count), whose
// matrices lie in the workspaces (window w_first first); S nested universes - the first sizes[s] columns - per workgroup
// from ONE factorisation at k.  All other arrays are indexed by the window's number in the batch.
//   conjugate (C != nullptr): C and T as tp_gram_launch stores them, t = X'1; n0 and w0 are the caller's priors.
//   Jeffreys  (C == nullptr): T holds M (T - t t'/N or the flagged form) as the run kernel keeps it, t its right-hand side;
//                             P = 1, n0 = w0 = nullptr.
struct tp_size_sweep_kargs_t {
    const double* C;            // [w_count x k x k], or nullptr: Jeffreys
    const double* T;            // [w_count x k x k]
    const double* t;            // [W x k]
    const double* n0;           // [W x P]
    const double* w0;           // [W x P x S x k]; entries at or beyond sizes[s] are never read
    const int* hf_count;        // optional [W]: intraday rows of the window (else m)
    const int* sizes;           // [S], strictly increasing within [1, k] (device memory)
    double* weights;            // [W x P x S x k]; entries at or beyond sizes[s] are written as 0
    int* status;                // [W x P x S]
    double* aux;                // [W x P x S x 8]: n0, n1, c, q0, q1, n1 - q1, 0, 0 (Jeffreys: 0, 0, 0, 0, q1, 0, 0, 0)
    long long w_first, w_count;
    int k, P, S, N, m;
    double gamma;
};
size_t tp_size_sweep_lds_bytes(int k, int S, bool conjugate);
hipError_t tp_size_sweep_launch(const tp_size_sweep_kargs_t& a, hipStream_t stream);
