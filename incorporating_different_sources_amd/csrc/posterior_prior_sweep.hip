// posterior_prior_sweep.hip - prior sweep (tp_batch_prior_sweep): many conjugate priors (n0, w0) per window from ONE pair of
// Grams.
//
// The Gram pass (posterior_gram_nt.hip) has stored, per window of the sub-range, the centred unscaled intraday scatter C, the
// daily Gram T and t = X'1.  This kernel takes one workgroup per (window, prior); with a = n0 m/(m-1):
//
//     S1 = a C + T        v = C w0        q0 = a w0'v        c = 2 n0 / (g + sqrt(g^2 + 4 n0 q0)),  g = n0 + k + 2
//     w1 = S1^-1 (c a v + t)      q1 = w1'S1 w1      n1 = n0 + N      weights = (n1 + k + 2) w1 / (n1 - q1) / gamma
//
// One pass over C forms the packed lower triangle of S1 in LDS (one fma per element; posterior_sweep_solve.h has the layout,
// R = 1) and, in the same pass, v: the 32 lanes that walk row c of C keep a partial product each and meet in a fixed
// butterfly.  The right-hand side c a v + t rides along as the extra row of the L D L' factorisation, which leaves the forward
// substitution y~ behind: q1 = sum y~_j^2 / d_j.  A pivot at or below k 2^-52 of its diagonal element flags the pair NOT_PD.
// Wave 0 runs the back substitution, the rescale, status and aux.
//
// Every (window, prior) is computed by its own workgroup from C, T, t, the window's intraday row count and the prior alone,
// in an order of operations that depends on k only: the result does not depend on W, P, the prior's or the window's position
// or the sub-ranges of the host loop.  Workgroup barriers only, each reached by every thread; nothing spins.
#include "posterior_sweep_solve.h"
#include "posterior_prior_sweep.h"

namespace {

constexpr int PRIOR_WREGS = 5;          // w0 registers per lane of a 32-lane row group: k <= 32 * 5

__global__ void __launch_bounds__(SWEEP_THREADS) posterior_prior_sweep_kernel(const tp_prior_sweep_kargs_t A) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int tid = threadIdx.x;
    const int k = A.k, H = k + 1;
    // priors of one window sit next to each other in the grid: the P workgroups of a window read the same C and T
    const long long wl = (long long)blockIdx.x / A.P;
    const int p = (int)((long long)blockIdx.x - wl * A.P);
    if (wl >= A.w_count) return;
    const long long w = A.w_first + wl;
    const long long wp = w * A.P + p;
    const double* __restrict__ C = A.C + wl * (long long)k * k;
    const double* __restrict__ T = A.T + wl * (long long)k * k;
    const double* __restrict__ w0 = A.w0 + wp * k;
    const double n0 = A.n0[wp];
    const double mm = (double)(A.hf_count != nullptr ? A.hf_count[w] : A.m);
    const double ap = n0 * (mm / (mm - 1.0));            // ref:333, as the run kernels form it
    double* vbuf = lds + sweep_off(k, H);                // [k] v = C w0, behind the packed image
    double* floor = vbuf + k;                            // [k] pivot floors: k 2^-52 times the diagonal of S1
    const double rel = (double)k * 0x1p-52;

    // ---- load: column c of the lower triangle of S1 = a C + T from row c of the two symmetric matrices, and v_c = C[c][:] w0
    const int tx = tid & (SWEEP_TX - 1), ty = tid / SWEEP_TX;
    double w0r[PRIOR_WREGS];
#pragma unroll
    for (int q = 0; q < PRIOR_WREGS; ++q) {
        const int i = tx + SWEEP_TX * q;
        w0r[q] = i < k ? w0[i] : 0.0;
    }
    for (int c = ty; c < k; c += SWEEP_TY) {
        double* col = lds + sweep_off(c, H) - c;
        double part = 0.0;
#pragma unroll
        for (int q = 0; q < PRIOR_WREGS; ++q) {
            const int i = tx + SWEEP_TX * q;
            if (i < k) {
                const double cv = C[(long long)c * k + i];
                part = fma(cv, w0r[q], part);
                if (i >= c) {
                    const double sv = fma(ap, cv, T[(long long)c * k + i]);
                    col[i] = sv;
                    if (i == c) floor[c] = rel * sv;
                }
            }
        }
        // the 32 lanes of a row group are one half of a wavefront: these exchanges stay inside it
#pragma unroll
        for (int o = SWEEP_TX / 2; o > 0; o >>= 1) part += __shfl_xor(part, o, 64);
        if (tx == 0) vbuf[c] = part;
    }
    __syncthreads();

    // ---- q0, c and the right-hand side c a v + t as row k (every wavefront forms the same q0 in the same order)
    const int lane = tid & 63, wv = tid >> 6;
    double zp = 0.0;
#pragma unroll
    for (int q = 0; q < SWEEP_XREGS; ++q) {
        const int i = lane + 64 * q;
        if (i < k) zp = fma(w0[i], vbuf[i], zp);
    }
    const double q0 = ap * wave_sum64(zp);
    const double g = n0 + k + 2;
    const double cc = (2 * n0) / (g + sqrt(g * g + 4 * n0 * q0));       // ref:415-418
    const double ca = cc * ap;
    for (int c = tid; c < k; c += SWEEP_THREADS) lds[sweep_off(c, H) + (k - c)] = fma(ca, vbuf[c], A.t[w * k + c]);
    __syncthreads();

    // ---- factorisation with the right-hand side riding along (posterior_sweep_solve.h)
    // A pivot that is no more than k 2^-52 of its diagonal element is rounding noise: the matrix is singular to working
    // precision (a duplicate column leaves +-1 ulp there, not always <= 0).  (A NaN pivot is not "<=": it ends as NONFINITE)
    const bool notpd = sweep_ldl_factor(lds, k, H, tid, floor);

    // ---- wave 0: q1 = w1'S1 w1 = sum y~_j^2 / d_j (ref:574), back substitution, weights (ref:572-575, 836)
    bool bad = false;
    double q1 = 0.0, denom = 0.0;
    const double n1 = n0 + (double)A.N;
    if (wv == 0) {
        double qp = 0.0;
#pragma unroll
        for (int q = 0; q < SWEEP_XREGS; ++q) {
            const int j = lane + 64 * q;
            if (j < k) {
                const double* cj = lds + sweep_off(j, H) - j;
                qp += cj[k] * cj[k] / cj[j];
            }
        }
        q1 = wave_sum64(qp);
        denom = n1 - q1;
        double x[SWEEP_XREGS];
        sweep_back_substitute(lds, k, H, 0, lane, x);
        double* out = A.weights + wp * k;
#pragma unroll
        for (int q = 0; q < SWEEP_XREGS; ++q) {
            const int i = lane + 64 * q;
            if (i < k) {
                const double v = 1.0 / A.gamma * ((n1 + k + 2) * x[q] / denom);
                out[i] = v;
                if (!isfinite(v)) bad = true;
            }
        }
    }
    const int anybad = __syncthreads_or(bad ? 1 : 0);
    if (tid == 0) {
        int st = TP_KSTATUS_OK;
        if (notpd) st = TP_KSTATUS_NOT_PD;
        else if (anybad) st = TP_KSTATUS_NONFINITE;
        else if (!(denom > 0.0)) st = TP_KSTATUS_BAD_DENOM;
        A.status[wp] = st;
        double* ax = A.aux + wp * 8;
        ax[0] = n0; ax[1] = n1; ax[2] = cc; ax[3] = q0; ax[4] = q1; ax[5] = denom; ax[6] = 0.0; ax[7] = 0.0;
    }
}

}  // namespace

size_t tp_prior_sweep_lds_bytes(int k) { return sizeof(double) * ((size_t)k * (k + 3) / 2 + 2 * (size_t)k); }

hipError_t tp_prior_sweep_launch(const tp_prior_sweep_kargs_t& a, hipStream_t stream) {
    static_assert(SWEEP_MAX_K <= SWEEP_TX * PRIOR_WREGS, "prior registers per lane");
    static_assert(SWEEP_MAX_K <= 64 * SWEEP_XREGS, "solution registers per lane");
    if (a.k < 1 || a.k > SWEEP_MAX_K || a.P < 1 || a.w_count < 1) return hipErrorInvalidValue;
    const long long grid = a.w_count * (long long)a.P;
    if (grid > 0x7fffffffLL) return hipErrorInvalidValue;
    static std::atomic<unsigned long long> attr_done{0};      // one bit per device (tp_allow_dynamic_lds)
    { hipError_t e = tp_allow_dynamic_lds(attr_done, posterior_prior_sweep_kernel, (int)tp_prior_sweep_lds_bytes(SWEEP_MAX_K)); if (e != hipSuccess) return e; }
    hipLaunchKernelGGL(posterior_prior_sweep_kernel, dim3((unsigned)grid), dim3(SWEEP_THREADS), tp_prior_sweep_lds_bytes(a.k), stream, a);
    return hipGetLastError();
}

// Gram pass: dispatcher over the tile count NT = ceil((k+1)/16) (posterior_gram_nt.hip, one translation unit per tile count)
#define TP_DECL(NT) hipError_t tp_gram_launch_nt##NT(const tp_gram_kargs_t&, hipStream_t);
TP_DECL(1) TP_DECL(2) TP_DECL(3) TP_DECL(4) TP_DECL(5) TP_DECL(6) TP_DECL(7) TP_DECL(8) TP_DECL(9)
#undef TP_DECL

hipError_t tp_gram_launch(const tp_gram_kargs_t& g, hipStream_t stream) {
    if (g.in.k < 1 || g.in.k > SWEEP_MAX_K || g.in.w_count < 1 || g.in.w_count > 0x7ffffff0LL) return hipErrorInvalidValue;
    switch ((g.in.k + 1 + 15) / 16) {
#define TP_CASE(NT) case NT: return tp_gram_launch_nt##NT(g, stream);
        TP_CASE(1) TP_CASE(2) TP_CASE(3) TP_CASE(4) TP_CASE(5) TP_CASE(6) TP_CASE(7) TP_CASE(8) TP_CASE(9)
#undef TP_CASE
        default: return hipErrorInvalidValue;
    }
}
