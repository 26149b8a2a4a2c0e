// posterior_prior_sweep.h - internal interface between the sweeps of the C-ABI (tangency_sweep.cpp) and the two kernels of the
// prior sweep.
#pragma once
#include "posterior_kernels.h"

// prior sweep (tp_batch_prior_sweep), Gram pass (posterior_gram_nt.hip, dispatcher in posterior_prior_sweep.hip): one
// wavefront per window of [in.w_first, in.w_first + in.w_count) stores the window's centred, UNSCALED intraday scatter
// C = sum (y - ybar)(y - ybar)' and its daily Gram T = X'X (both k x k, symmetric, full storage, the sub-range's first
// window first) and t = X'1 (indexed by the window's number in the batch).  Reads the layout fields of `in` only - no
// prior, no shared block sums, no outputs of a run.  k <= tp_sweep_max_k().
struct tp_gram_kargs_t {
    tp_kargs_t in;
    double* C;                  // [w_count x k x k]
    double* T;                  // [w_count x k x k]
    double* t;                  // [W x k]
};
// hipErrorNotSupported: index layout with passes too long for the kernel's LDS staging (nothing was launched)
hipError_t tp_gram_launch(const tp_gram_kargs_t& g, hipStream_t stream);

// prior sweep, solve kernel (posterior_prior_sweep.hip): one workgroup per (window, prior) of the windows
// [w_first, w_first + w_count), whose C and T lie in the two workspaces (window w_first first).  All other arrays are indexed
// by the window's number in the batch.
struct tp_prior_sweep_kargs_t {
    const double* C;            // [w_count x k x k]
    const double* T;            // [w_count x k x k]
    const double* t;            // [W x k]
    const double* n0;           // [W x P]
    const double* w0;           // [W x P x k]
    const int* hf_count;        // optional [W]: intraday rows of the window (else m)
    double* weights;            // [W x P x k]
    int* status;                // [W x P]
    double* aux;                // [W x P x 8]: n0, n1, c, q0, q1, n1 - q1, 0, 0
    long long w_first, w_count;
    int k, P, N, m;
    double gamma;
};
size_t tp_prior_sweep_lds_bytes(int k);
hipError_t tp_prior_sweep_launch(const tp_prior_sweep_kargs_t& a, hipStream_t stream);

// prior sweep on the large-k tiled path (posterior_prior_sweep_tiled.hip, tp_batch_prior_sweep_tiled): fills e_count arena
// entries - entry e is the (window, prior) pair with the flat index e_first + e = w P + p - with a C + T, the border column
// c a C w0 + t, ws.scal and ws.flags, as tiled_clear_kernel leaves a conjugate window; tp_tiled_factor_launch takes it from
// there.  C and T are those of the windows [wc_first, ..) of the sub-range (symmetric, full storage); t, n0, w0 and hf_count
// are indexed by the numbers in the batch.  Uses ws.arena, ws.part [e_count][NS][NS][64], ws.ybar (scratch), ws.scal, ws.flags.
struct tp_prior_sweep_tiled_kargs_t {
    const double* C;            // [windows of the sub-range x k x k]
    const double* T;            // [windows of the sub-range x k x k]
    const double* t;            // [W x k]
    const double* n0;           // [W x P]
    const double* w0;           // [W x P x k]
    const int* hf_count;        // optional [W]: intraday rows of the window (else m)
    long long e_first, e_count; // e_count <= the workspace's capacity
    long long wc_first;         // first window of the sub-range
    int k, P, m;
};
hipError_t tp_prior_sweep_tiled_launch(const tp_prior_sweep_tiled_kargs_t& a, const tp_tiled_ws_t& ws, hipStream_t stream);
