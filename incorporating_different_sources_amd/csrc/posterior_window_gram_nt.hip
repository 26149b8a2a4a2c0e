// posterior_window_gram_nt.hip - Gram pass of the window sweep (tp_batch_window_sweep) for one tile count TP_NT: ONE wavefront
// per window on the one-wave kernel's row loop wave_gram (posterior_wave_impl.h), as the prior sweep's Gram pass
// (posterior_gram_nt.hip) uses it.
//
// Conjugate: the intraday pass and the store of the centred, unscaled scatter C exactly as there, once per window - no length
// changes the intraday rows (ref:299-314).  Then the daily rows go through the MFMAs from the newest backwards: the
// accumulators are cleared once and wave_gram is called per segment - segment 0 the last rows[0] rows, segment l the positions
// [n_w - rows[l], n_w - rows[l-1]) - with the row source advanced by the segment's offset.  After segment l the accumulators
// hold T_l = X_l'X_l and, in the border column, t_l = X_l'1 over the last rows[l] rows: both are stored and nothing is
// cleared.  A snapshot is a store, not more flops: every daily row passes the MFMAs once whatever L is.  wave_gram masks a
// k-step that runs past its count, so a segment of any length >= 1 is legal; an empty one (a tie) is skipped.
// A row older than a length's suffix is loaded after that length's snapshot has left the registers: it cannot reach it.
#include "posterior_wave_impl.h"
#include "posterior_window_sweep.h"

#ifndef TP_NT
#error "compile with -DTP_NT=<tiles per side>"
#endif
#define TP_CAT2(a, b) a##b
#define TP_CAT(a, b) TP_CAT2(a, b)

namespace {

// LDS image: [KP] column sums of the centring, then (general layout) the staged rows of the pass in flight
constexpr int WGRAM_LDS_LIMIT = 128 * 1024;

template <int NT, bool LEAN, bool CONJ>
__device__ __forceinline__ void window_gram_body(const tp_window_gram_kargs_t& G, double* lds) {
    const tp_kargs_t& A = G.in;
    constexpr int KP = 16 * NT;
    constexpr int NTILES = NT * (NT + 1) / 2;
    constexpr int OFF_VEC = 0, OFF_SUB = KP;
    const int lane = threadIdx.x;
    const int fr = lane & 15, fq = lane >> 4;
    const int k = A.k;
    __builtin_assume(k >= 16 * (NT - 1));
    __builtin_assume(k <= 16 * NT - 1);
    constexpr int kI = NT - 1;
    const int kc = k - 16 * kI;
    // XCD-aware workgroup -> window map (see posterior_fused_impl.h): one contiguous window range per XCD
    const long long per_xcd = (A.w_count + 7) >> 3;
    const long long wl = (long long)(blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3);
    if ((long long)(blockIdx.x >> 3) >= per_xcd || wl >= A.w_count) return;
    const long long w = A.w_first + wl;

    const int* cols = (!LEAN && A.col_idx) ? A.col_idx + w * k : nullptr;
    long long coff[NT];
    if (cols != nullptr) {
        int cidx[NT];
#pragma unroll
        for (int i = 0; i < NT; ++i) {
            const int c = 16 * i + fr;
            cidx[i] = cols[c < k ? c : k - 1];
        }
#pragma unroll
        for (int i = 0; i < NT; ++i) coff[i] = (long long)cidx[i];
    } else {
#pragma unroll
        for (int i = 0; i < NT; ++i) {
            const int c = 16 * i + fr;
            coff[i] = (long long)(c < k ? c : k - 1);
        }
    }
    double* idx_sub_lds = LEAN ? nullptr : lds + OFF_SUB;
    int* idx_rows_lds = LEAN ? nullptr : (int*)(lds + OFF_SUB + wave_idx_rows(A.n_r, A.m, CONJ));
    d4 acc[NTILES];
    static_for<0, NTILES>([&](auto tc) __attribute__((always_inline)) { acc[decltype(tc)::value] = d4{0.0, 0.0, 0.0, 0.0}; });
    wave_pin(acc);

    // (this block is gram_window_body's intraday pass and centring, posterior_gram_nt.hip, which must keep its instruction
    // stream and is therefore not shared: keep the two in step)
    if constexpr (CONJ) {
        double* const Cw = G.C + wl * (long long)k * k;
        WRows hs;
        hs.base = A.hf_panel; hs.ld = A.hf_ld;
        hs.ridx = (!LEAN && A.hf_row_idx) ? A.hf_row_idx + w * (long long)A.m : nullptr;
        hs.first = A.hf_start ? A.hf_start[w] : 0;
        hs.sub_row = nullptr;
        hs.count = A.hf_count ? A.hf_count[w] : A.m;
        hs.count0 = 0x7fffffff; hs.jump = 0;
        hs.off32 = (A.hf_off32 & 1) != 0;
        // ---- the shift row of the one-pass centred scatter = the window's first row (posterior_wave_impl.h, phase A)
        const bool ones = kc < 15;        // a spare column k+1 carries ones; otherwise the sums are kept by vector adds (wave_gram)
        double shift[NT], w0v[NT], csum[NT];
        double usum = 0.0;
        {
            const long long row0 = hs.ridx ? (long long)hs.ridx[0] : hs.first;
            const double* p0 = hs.base + row0 * (long long)hs.ld;
#pragma unroll
            for (int i = 0; i < NT; ++i) {
                shift[i] = p0[coff[i]];      // raw: zeroed beyond column k inside wave_gram (lazy_mask)
                w0v[i] = 0.0;                // no prior here: column k of the bordered matrix stays zero
                csum[i] = 0.0;
            }
        }
        // ---- Gram of the shifted intraday rows (phase B); the first row, shifted, is exactly zero: the pass starts at row 1
        const int hf_rows_all = hs.count;
        if (!hs.ridx) { hs.first += 1; hs.count -= 1; }
        else { hs.ridx += 1; hs.count -= 1; }
        if constexpr (!LEAN) wave_stage_rows(hs, lane, idx_rows_lds, idx_sub_lds);
        wave_gram<NT, 1, 0, true, LEAN>(hs, coff, k, lane, shift, w0v, ones, true, acc, idx_rows_lds, idx_sub_lds, csum, usum);
        hs.count = hf_rows_all;
        // ---- rank-one term of the centring (phase C without the scaling): C_ij = G_ij - s_i s_j / m
        const double invm = 1.0 / (double)hs.count;
        double tj[NT];
        if (ones) {
            static_for<0, NT>([&](auto Ic) __attribute__((always_inline)) {
                constexpr int I = decltype(Ic)::value;
                constexpr int t = wtile(NT, I, kI);
                if (fr == kc + 1) {
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        lds[OFF_VEC + 16 * I + fq + 4 * r] = (I < kI || fq + 4 * r <= kc) ? acc[t][r] : 0.0;
                }
            });
        } else {
#pragma unroll
            for (int i = 0; i < NT; ++i) {
                double sc_ = csum[i];
                sc_ += __shfl_xor(sc_, 16, 64);
                sc_ += __shfl_xor(sc_, 32, 64);
                if (fq == 0) lds[OFF_VEC + 16 * i + fr] = (16 * i + fr < k) ? sc_ : 0.0;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int J = 0; J < NT; ++J) tj[J] = lds[OFF_VEC + 16 * J + fr];
        static_for<0, NT>([&](auto Ic) __attribute__((always_inline)) {
            constexpr int I = decltype(Ic)::value;
            double ti[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) ti[r] = -(lds[OFF_VEC + 16 * I + fq + 4 * r] * invm);
            static_for<I, NT>([&](auto Jc) __attribute__((always_inline)) {
                constexpr int J = decltype(Jc)::value;
                constexpr int t = wtile(NT, I, J);
                d4 x = acc[t];
#pragma unroll
                for (int r = 0; r < 4; ++r) x[r] = fma(ti[r], tj[J], x[r]);
                wave_post_tile<I, J>(Cw, k, fr, fq, x);
                acc[t] = d4{0.0, 0.0, 0.0, 0.0};
                wave_pin1<t>(acc[t]);
            });
            __builtin_amdgcn_sched_barrier(0);
        });
        __builtin_amdgcn_wave_barrier();
    }
    // ---- daily Gram (ref:180) + t in the border column (ref:222), newest segment first: every row through the MFMAs once,
    // a snapshot after every segment
    const int L = G.L;
    const int* rw = G.rows + w * (long long)L;
    const int n_w = A.n_rows ? A.n_rows[w] : A.n_r;
    const int* const ridx0 = (!LEAN && A.row_idx) ? A.row_idx + w * (long long)A.n_r : nullptr;
    const long long first0 = A.start ? A.start[w] : 0;
    const double* const sub0 = A.rf_adj ? A.rf_adj + w * (long long)A.n_r : nullptr;
    double* const Tw = G.T + wl * (long long)L * k * k;
    double* const tw = G.t + w * (long long)L * k;
    int done = 0;                             // rows of the suffix that are in the accumulators
    int l = 0;
#pragma nounroll
    while (l < L) {
        // rows[l] > done here: the first length has at least one row, and the lengths tied with a snapshot left with it below
        const int rl = rw[l];
        wave_pin(acc);
        {
            const int off = n_w - rl;
            WRows ds;
            ds.base = A.panel; ds.ld = A.panel_ld;
            ds.ridx = ridx0 ? ridx0 + off : nullptr;
            ds.first = first0 + off;
            ds.sub_row = sub0 ? sub0 + off : nullptr;
            ds.count = rl - done;
            ds.count0 = 0x7fffffff; ds.jump = 0;
            ds.off32 = (A.panel_off32 & 1) != 0;
            double none[NT] = {};
            // (every load of the pass before has been consumed when wave_gram returned: its staging region is free)
            if constexpr (!LEAN) wave_stage_rows(ds, lane, idx_rows_lds, idx_sub_lds);
            double nosum = 0.0;
            wave_gram<NT, 1, 0, false, LEAN>(ds, coff, k, lane, none, none, false, false, acc, idx_rows_lds, idx_sub_lds, none, nosum);
            done = rl;
        }
        wave_pin(acc);
        // the snapshot, once per length that ends here (a tie is an empty segment: the same registers go out again)
#pragma nounroll
        do {
            double* const P = Tw + (long long)l * k * k;
            static_for<0, NT>([&](auto Ic) __attribute__((always_inline)) {
                constexpr int I = decltype(Ic)::value;
                static_for<I, NT>([&](auto Jc) __attribute__((always_inline)) {
                    constexpr int J = decltype(Jc)::value;
                    wave_post_tile<I, J>(P, k, fr, fq, acc[wtile(NT, I, J)]);
                });
            });
            static_for<0, NT>([&](auto Ic) __attribute__((always_inline)) {
                constexpr int I = decltype(Ic)::value;
                constexpr int t = wtile(NT, I, kI);
                if (fr == kc) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int gi = 16 * I + fq + 4 * r;
                        if (gi < k) tw[(long long)l * k + gi] = acc[t][r];
                    }
                }
            });
            ++l;
        } while (l < L && rw[l] <= done);
    }
}

template <int NT, bool LEAN, bool CONJ>
__global__ void __launch_bounds__(64, wave_occupancy(NT)) posterior_window_gram_kernel(const tp_window_gram_kargs_t G) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    window_gram_body<NT, LEAN, CONJ>(G, lds);
}

template <int NT, bool LEAN, bool CONJ>
hipError_t window_gram_launch_variant(const tp_window_gram_kargs_t& g, hipStream_t stream) {
    const int lds_bytes = 16 * NT * 8 + (LEAN ? 0 : wave_idx_bytes(g.in.n_r, g.in.m, CONJ));
    if (lds_bytes > WGRAM_LDS_LIMIT) return hipErrorNotSupported;
    static std::atomic<unsigned long long> attr_done{0};      // one bit per device (tp_allow_dynamic_lds)
    { hipError_t e = tp_allow_dynamic_lds(attr_done, posterior_window_gram_kernel<NT, LEAN, CONJ>, WGRAM_LDS_LIMIT); if (e != hipSuccess) return e; }
    const int grid8 = 8 * (int)((g.in.w_count + 7) / 8);
    hipLaunchKernelGGL((posterior_window_gram_kernel<NT, LEAN, CONJ>), dim3(grid8), dim3(64), lds_bytes, stream, g);
    return hipGetLastError();
}

}  // namespace

hipError_t TP_CAT(tp_window_gram_launch_nt, TP_NT)(const tp_window_gram_kargs_t& g, hipStream_t stream) {
    const bool lean = tp_layout_is_lean(g.in);
    if (g.C != nullptr)
        return lean ? window_gram_launch_variant<TP_NT, true, true>(g, stream) : window_gram_launch_variant<TP_NT, false, true>(g, stream);
    return lean ? window_gram_launch_variant<TP_NT, true, false>(g, stream) : window_gram_launch_variant<TP_NT, false, false>(g, stream);
}
