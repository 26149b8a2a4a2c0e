// posterior_tiled_window_wave.h - the segmented Gram of the tiled window sweep (tp_batch_window_sweep_tiled): ONE wavefront per
// (window, 64 x 64 super-tile), every daily row through the MFMAs once whatever the number of lengths.
// Included by posterior_tiled.hip behind posterior_tiled_wave.h, whose row loop tw_gram_pass it runs.
//
// The 16 tiles of the super-tile (128 AGPRs) are cleared once.  The daily rows go through tw_gram_pass<.., HF = false> from
// the newest backwards in L segments - segment 0 the last rows[w][0] positions of the window, segment l the positions
// [n_w - rows[w][l], n_w - rows[w][l-1]) - with the row source (first / ridx, rowc = the risk-free adjustment) advanced by the
// segment's offset.  After segment l the accumulators hold this super-tile's part of T_l = X_l'X_l and, in the border (ones)
// column of the last super-tile column, of t_l = X_l'1 over the last rows[w][l] rows: both go out by ordinary vector stores and
// nothing is cleared.  A snapshot is a store, not more flops.
//
// The MFMA loop is never called conditionally inside the segment loop (a conditional call puts the accumulators
// through a phi and the register allocator through copies): a tie - equal rows for several lengths - is an empty segment, so
// the inner loop stores the same registers once per tied length and the outer loop goes on with the next length that has more
// rows.  Every segment that reaches tw_gram_pass has at least one row (the count is clamped to 1: the compiler drops the
// pass's early return, and with it the second version of the accumulators; DESIGN.md 4m has what the listing shows).
// A row older than a length's suffix is loaded after that length's snapshot has left the registers: it cannot reach it.
// Both loops are bounded by L; the row loop by the segment's row count.
#include "posterior_window_sweep.h"

template <bool DIAG, bool EDGE>
__device__ __forceinline__ void window_gram64_wave_body(const tp_window_gram_kargs_t& G, const long long wl, const int SI, const int SJ) {
    constexpr int NB = 4, NC = 8;
    const tp_kargs_t& A = G.in;
    const int lane = threadIdx.x;
    const int fr = lane & 15, fq = lane >> 4;
    const long long w = A.w_first + wl;
    const int k = A.k;
    const int* cols = A.col_idx ? A.col_idx + w * k : nullptr;

    int co[NC];
    double yb[NC], cs[NC];
    bool cval[NC], cbord[NC];
#pragma unroll
    for (int i = 0; i < NC; ++i) {
        // operand groups as in gram64_wave_body: 0..3 the A groups (super-tile column SI), 4..7 the B groups of SJ
        const int st = DIAG ? SI + (i >> 2) : (i < 4 ? SI : SJ + ((i - 4) >> 2));
        const int gc = 64 * st + fr + 16 * (i & 3);
        cval[i] = !EDGE || gc < k;
        cbord[i] = EDGE && gc == k;
        const int gcl = cval[i] ? gc : k - 1;                      // padding columns re-read column k-1 (masked)
        co[i] = cols ? cols[gcl] : gcl;
        yb[i] = 0.0; cs[i] = 0.0;
    }
    d4 acc[4 * NB];
    static_for<0, 4 * NB>([&](auto tc) __attribute__((always_inline)) {
        acc[decltype(tc)::value] = d4{0.0, 0.0, 0.0, 0.0};
        tw_pin1(acc[decltype(tc)::value]);
    });

    const int L = G.L;
    const int* rw = G.rows + w * (long long)L;
    const int n_w = A.n_rows ? A.n_rows[w] : A.n_r;
    const int* const ridx0 = A.row_idx ? A.row_idx + w * (long long)A.n_r : nullptr;
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
        {
            const int off = n_w - rl;
            const int cnt = rl - done;
            TRows ds;
            ds.base = A.panel; ds.ld = A.panel_ld;
            ds.ridx = ridx0 ? ridx0 + off : nullptr;
            ds.first = first0 + off;
            ds.rowc = sub0 ? sub0 + off : nullptr;
            ds.count = cnt > 0 ? cnt : 1;                          // (host-checked: always cnt)
            ds.count0 = 0x7fffffff; ds.jump = 0;
            tw_gram_pass<DIAG, EDGE, false, NB>(ds, co, yb, cval, cbord, 0.0, lane, acc, cs);
            done = rl;
        }
        // the snapshot, once per length that ends here (a tie is an empty segment: the same registers go out again)
#pragma nounroll
        do {
            double* const P = Tw + (long long)l * k * k;
            double* const tl = tw + (long long)l * k;
            static_for<0, 4>([&](auto ac) __attribute__((always_inline)) {
                constexpr int a = decltype(ac)::value;
                static_for<0, NB>([&](auto bc) __attribute__((always_inline)) {
                    constexpr int b = decltype(bc)::value;
                    if constexpr (!DIAG || a <= b) {               // (a diagonal super-tile: column >= row is all that is read)
                        const d4 x = acc[NB * a + b];
                        const int gj = 64 * SJ + 16 * b + fr;
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int gi = 64 * SI + 16 * a + fq + 4 * r;
                            if (!EDGE || (gi < k && gj < k)) P[(long long)gi * k + gj] = x[r];
                            if (EDGE && gj == k && gi < k) tl[gi] = x[r];      // ones column: t_l for the asset rows of SI
                        }
                    }
                });
                __builtin_amdgcn_sched_barrier(0);
            });
            ++l;
        } while (l < L && rw[l] <= done);
    }
}

__global__ void __launch_bounds__(64, 2) tiled_window_gram_wave_kernel(const tp_window_gram_kargs_t G, const int NS) {
    long long wl;
    int tile, SI, SJ;
    if (!xcd_window_tile(NS * (NS + 1) / 2, G.in.w_count, wl, tile)) return;
    pair_decode(tile, NS, SI, SJ);
    const bool edge = !(64 * SJ + 63 < G.in.k);                   // SI <= SJ: otherwise every column is a real asset
    if (SI == SJ) {
        if (edge) window_gram64_wave_body<true, true>(G, wl, SI, SJ);
        else window_gram64_wave_body<true, false>(G, wl, SI, SJ);
    } else {
        if (edge) window_gram64_wave_body<false, true>(G, wl, SI, SJ);
        else window_gram64_wave_body<false, false>(G, wl, SI, SJ);
    }
}

// One wave per (window, super-tile) of the windows [in.w_first, in.w_first + in.w_count).  g.C is not read: the intraday
// scatter of a conjugate tiled window sweep comes from the batch's own tiled Gram stage.
hipError_t tp_tiled_window_gram_launch(const tp_window_gram_kargs_t& g, hipStream_t stream) {
    if (g.in.k <= 0 || g.in.k > tp_tiled_max_assets() || g.L < 1 || g.in.w_count < 1 || g.T == nullptr || g.t == nullptr || g.rows == nullptr)
        return hipErrorInvalidValue;
    int KP, NS, NSB;
    tp_tiled_geometry(g.in.k, &KP, &NS, &NSB);
    const long long blocks = ((g.in.w_count + 7) / 8) * 8 * (long long)(NS * (NS + 1) / 2);
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(tiled_window_gram_wave_kernel, xcd_grid(NS * (NS + 1) / 2, g.in.w_count), dim3(64), 0, stream, g, NS);
    return hipGetLastError();
}
