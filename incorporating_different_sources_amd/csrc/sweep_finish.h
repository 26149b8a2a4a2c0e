// sweep_finish.h - interface between the host layer (tangency_sweep.cpp) and the sweep finish kernels (sweep_finish.hip):
// the Greyserman and Jorion weights from the solutions a solve sweep (S shifts, R = 2 right-hand sides [t, 1]) left on the device.
#pragma once
#include <hip/hip_runtime.h>

#define TP_FINISH_DRAWS_PER_WAVE 16  // consecutive shifts of ONE window per wavefront (TP_FINISH_DRAWS_PER_WAVE of the C-ABI)
#define TP_FINISH_MAX_SLOTS 32       // columns per lane: 64 x 32 = 2048 >= the largest k a tiled sweep with R = 2 serves
#define TP_FINISH_KMODE_GREYSERMAN 0
#define TP_FINISH_KMODE_JORION 1
#define TP_FINISH_KSTATUS_NONFINITE 2

struct tp_finish_args_t {
    const double* x;                 // [W x S x 2 x k] the sweep's solutions: slot 0 for t, slot 1 for the ones vector
    const int* xstatus;              // [W x S]
    const double* t;                 // [W x k] the sweep's default right-hand sides
    const double* n;                 // [W]
    const double* kappa;             // [W] (Greyserman)
    const double* hyper;             // [W x S x 2] (xi, eta) (Greyserman)
    double* part;                    // [W x NG x k] the groups' partial sums, NG = ceil(S / TP_FINISH_DRAWS_PER_WAVE)
    int* gstatus;                    // [W x NG] the first non-OK xstatus of each group
    double* weights;                 // [W x k]
    int* status;                     // [W]
    double* aux;                     // [W x S x 4]
    double gamma;
    int W, S, k, mode;
};

// The scalar algebra of TP_FINISH_GREYSERMAN, shared with the spectral sweep (posterior_spectral.hip): one rounding per
// operation, in the order include/tangency_posterior.h documents.  c = tp_finish_greyserman_scale(gamma, N, n).
struct tp_finish_coeffs_t { double det, cA, cB; };

__device__ __forceinline__ double tp_finish_greyserman_scale(double gamma, double N, double n) {
    return ((1 / gamma) * ((N + n) + 1)) * (1 - 1 / n);
}

__device__ __forceinline__ tp_finish_coeffs_t tp_finish_greyserman_coeffs(double s1, double s2, double s3, double n, double kappa,
                                                                          double xi, double eta, double c) {
    const double beta = eta / 2 + kappa * (xi * xi);
    const double K11 = 1 / beta + s1;
    const double K12 = s2 - (kappa * xi) / beta;
    const double K22 = (s3 - n) - (kappa * eta) / (2 * beta);
    tp_finish_coeffs_t r;
    r.det = K11 * K22 - K12 * K12;
    r.cA = c * (K12 / r.det);
    r.cB = c * (K11 / r.det);
    return r;
}

// the partial sums of every (window, group), then every window's weights and status: two launches on `st`
hipError_t tp_finish_launch(const tp_finish_args_t& a, hipStream_t st);
