// posterior_spectral.h - interface between the host layer (tangency_sweep.cpp) and the spectral ridge sweep
// (posterior_spectral.hip): the Greyserman weights of S ridge shifts per window from ONE eigendecomposition of the window's
// matrix instead of S factorisations.  k <= tp_sweep_max_k().
#pragma once
#include <hip/hip_runtime.h>

#define TP_SPECTRAL_KMAX_SWEEPS 32        // TP_SPECTRAL_MAX_SWEEPS of the C-ABI
#define TP_SPECTRAL_KSTATUS_NO_CONVERGENCE 4   // TP_STATUS_NO_CONVERGENCE of the C-ABI

struct tp_spectral_args_t {
    const double* post;              // [w_count x k x k] the matrices M of the sub-range, as the Gram pass stored them
    const double* t;                 // [W x k] the Gram pass's default right-hand sides
    double* V;                       // eigenvectors, column-major k x k per window: window w_first + i at V + (v_first + i) k k
    double* lambda;                  // [W x k] eigenvalues (not sorted)
    double* that;                    // [W x k] V't
    double* ohat;                    // [W x k] V'1
    int* sweeps;                     // [W] Jacobi sweeps performed, the last one (without a rotation) included
    int* jstatus;                    // [W] 0, TP_KSTATUS_NONFINITE (input) or TP_SPECTRAL_KSTATUS_NO_CONVERGENCE
    const double* n;                 // [W]
    const double* kappa;             // [W]
    const double* hyper;             // [W x S x 2] (xi, eta)
    double* part;                    // [W x NG x k] the groups' partial sums in the eigenbasis, NG = ceil(S / TP_FINISH_DRAWS_PER_WAVE)
    int* gstatus;                    // [W x NG] the first non-OK shift status of each group
    double* weights;                 // [W x k]
    int* status;                     // [W]
    double* aux;                     // [W x S x 4]
    double gamma;
    long long w_first, w_count;      // the sub-range
    long long v_first;               // where the sub-range starts in V: w_first when every window's V is kept, else 0
    int S, k;
};

// dynamic LDS of spectral_jacobi_kernel: the packed lower triangle with two extra rows
size_t tp_spectral_lds_bytes(int k);
// the three launches of one sub-range on `st`: eigendecompositions, partial sums of every (window, group), weights and statuses
hipError_t tp_spectral_launch(const tp_spectral_args_t& a, hipStream_t st);
