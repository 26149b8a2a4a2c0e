// posterior_window_sweep.h - internal interface between the sweeps of the C-ABI (tangency_sweep.cpp) and the three kernels of
// the window sweep (tp_batch_window_sweep): the segmented Gram pass (posterior_window_gram_nt.hip, dispatcher in
// posterior_window_sweep.hip), the delta kernel and the solve kernel (posterior_window_sweep.hip) - and, at the end, the kernels
// of its large-k form (tp_batch_window_sweep_tiled): the segmented one-wave Gram of posterior_tiled.hip and the fill kernels of
// posterior_window_sweep_tiled.hip.  The delta kernel serves both.
#pragma once
#include "posterior_kernels.h"

// window sweep, Gram pass: one wavefront per window of [in.w_first, in.w_first + in.w_count).  Conjugate (C != nullptr): the
// centred, UNSCALED intraday scatter C as tp_gram_launch stores it, once.  Then the daily rows from the newest backwards in L
// segments - segment l: the positions [n_w - rows[w][l], n_w - rows[w][l-1]) - into accumulators that are cleared once; after
// segment l the snapshot T_l = sum x x' (k x k, symmetric, full storage) and t_l = sum x over the last rows[w][l] rows go out.
// Reads the layout fields of `in` only.  k <= tp_sweep_max_k().
struct tp_window_gram_kargs_t {
    tp_kargs_t in;
    double* C;                  // [w_count x k x k], or nullptr: Jeffreys, no intraday pass
    double* T;                  // [w_count x L x k x k]
    double* t;                  // [W x L x k]
    const int* rows;            // [W x L] non-decreasing in l, within [1, n_w] (device memory)
    int L;
};
// hipErrorNotSupported: index layout with passes too long for the kernel's LDS staging (nothing was launched)
hipError_t tp_window_gram_launch(const tp_window_gram_kargs_t& g, hipStream_t stream);

// window sweep, delta kernel: one workgroup per (window, length) of the windows [in.w_first, in.w_first + in.w_count), one
// thread per column (k > 192: a thread takes every 192nd column).  Over the last rows[w][l] positions r of the window, oldest
// first, with x_r the batch's own row (panel - rf_adj):  dv[w][l][j] = sum_r delta[w][l][r] x_rj ,  ds[w][l] = (sum_r delta_r, sum_r delta_r^2).
struct tp_window_delta_kargs_t {
    tp_kargs_t in;
    const double* delta;        // [W x L x n_r], indexed by the position in the window
    const int* rows;            // [W x L]
    double* dv;                 // [W x L x k]
    double* ds;                 // [W x L x 2]
    int L;
};
hipError_t tp_window_delta_launch(const tp_window_delta_kargs_t& a, hipStream_t stream);

// window sweep, solve kernel: one workgroup per (window, prior, length) of the windows [w_first, w_first + w_count), whose C
// and snapshots lie in the workspaces (window w_first first).  All other arrays are indexed by the window's number in the batch.
//   conjugate (C != nullptr): n0 and w0 are the caller's priors.
//   Jeffreys  (C == nullptr): P = 1, n0 = w0 = nullptr; center_rows as tp_kargs_t (0: / N[l], 1: / rows[w][l], 2: no term).
struct tp_window_sweep_kargs_t {
    const double* C;            // [w_count x k x k], or nullptr: Jeffreys
    const double* T;            // [w_count x L x k x k]
    const double* t;            // [W x L x k]
    const double* dv;           // [W x L x k], or nullptr: no delta
    const double* ds;           // [W x L x 2], or nullptr
    const double* n0;           // [W x P x L]
    const double* w0;           // [W x P x k]
    const int* hf_count;        // optional [W]: intraday rows of the window (else m)
    const int* rows;            // [W x L]
    const int* N;               // [L] (device memory)
    double* weights;            // [W x P x L x k]
    int* status;                // [W x P x L]
    double* aux;                // [W x P x L x 8]: n0, n1, c, q0, q1, n1 - q1, 0, 0 (Jeffreys: 0, 0, 0, 0, q1, 0, 0, 0)
    long long w_first, w_count;
    int k, P, L, m, center_rows;
    double gamma;
};
size_t tp_window_sweep_lds_bytes(int k);
hipError_t tp_window_sweep_launch(const tp_window_sweep_kargs_t& a, hipStream_t stream);

// ---- the window sweep above tp_sweep_max_k() (tp_batch_window_sweep_tiled), on the large-k tiled pipeline ----------------

// segmented Gram (posterior_tiled_window_wave.h, built into posterior_tiled.hip): one wavefront per (window, 64 x 64
// super-tile I <= J) of the windows [in.w_first, in.w_first + in.w_count).  The daily rows as above, newest segment first; after
// segment l the super-tile's part of T_l (row-major k x k, column >= row only) and, from the last super-tile column, the asset
// rows of t_l go out.  g.C is not read.  k <= tp_tiled_max_assets().
hipError_t tp_tiled_window_gram_launch(const tp_window_gram_kargs_t& g, hipStream_t stream);

// fill of the arena entries (posterior_window_sweep_tiled.hip).  The entries of ONE launch share the length l: entry e is the
// (window, prior) pair wp_first + e, wp = w P + p, of the windows whose matrices start at window wc_first in C and T.
struct tp_window_sweep_tiled_kargs_t {
    const double* C;            // [chunk x k x k] symmetric, full storage, or nullptr: Jeffreys
    const double* T;            // [chunk x L x k x k], column >= row valid
    const double* t;            // [W x L x k]
    const double* dv;           // [W x L x k], or nullptr: no delta
    const double* ds;           // [W x L x 2], or nullptr
    const double* n0;           // [W x P x L]
    const double* w0;           // [W x P x k]
    const int* hf_count;        // optional [W]: intraday rows of the window (else m)
    const int* rows;            // [W x L]
    double* cw;                 // [chunk x P x k] C w0 of the sub-range's (window, prior) pairs
    double* cq;                 // [chunk x P] w0'C w0
    // results: the staging rows of the launch's entries (written by tp_tiled_factor_launch) go to their slots (wp L + l)
    const double* stage_w; const int* stage_s; const double* stage_a;
    double* weights; int* status; double* aux;
    long long wc_first;         // first window of the sub-range
    long long wp_first, e_count;
    int k, P, L, l, m, N, center_rows;
};
// C w0 and w0'C w0 for the pairs [wp_first, wp_first + e_count): once per (window, prior), whatever L is
hipError_t tp_window_sweep_tiled_cw_launch(const tp_window_sweep_tiled_kargs_t& a, hipStream_t stream);
// arena, ws.scal = (s, sqrt s, c, q0, n0) and ws.flags of the launch's entries, as tiled_clear_kernel leaves them for a run
hipError_t tp_window_sweep_tiled_fill_launch(const tp_window_sweep_tiled_kargs_t& a, const tp_tiled_ws_t& ws, hipStream_t stream);
// staging rows -> result slots
hipError_t tp_window_sweep_tiled_scatter_launch(const tp_window_sweep_tiled_kargs_t& a, hipStream_t stream);
