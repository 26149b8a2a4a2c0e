#pragma once
// posterior_wave_impl.h - ONE wavefront per rolling window (register-tile path, small tile counts).
//
// The multi-wave kernel of posterior_fused_impl.h spreads the tiles of a window over 4 waves: every staged row
// goes global -> registers -> LDS -> MFMA operand, every phase ends at a workgroup barrier, and during the
// serial phases (the 16-pivot elimination of a diagonal tile, the back substitution) three of the four waves
// of a window are parked (61 % of all wave cycles, profiles/r02_final_pmc_stall_fused_k100.txt).
//
// Here a window is ONE wave that owns the whole upper triangle of the bordered matrix (NT (NT+1)/2 accumulator
// tiles = 224 registers at NT = 7, in the 512-entry unified VGPR/AGPR file at one wave per SIMD):
//   * the MFMA operands of a 4-row k-step are loaded straight from the panels: lane (fq, fr) reads row 4s+fq,
//     column 16i+fr - one 8-byte load per 16-column group IS the A/B operand of every tile in that tile row /
//     column.  No LDS staging, no barrier, three k-steps of loads in flight;
//   * register r of an accumulator tile holds rows 4r..4r+3 of the tile in exactly the MFMA operand layout, so
//     the block row R_jJ = M A_jJ and the trailing update A_IJ -= R_jI' R_jJ of the blocked Cholesky take their
//     operands from the accumulators themselves - the factorisation touches LDS only for the 16x16 diagonal
//     tile (to turn it into one column per lane for the pivot chain, and to broadcast a pivot's multipliers) and for
//     M = R_jj^-T;
//   * the back substitution runs along block ROWS: lane-local products over the tiles of the row, one 16-lane
//     DPP reduction per register, and w_I = M' z by MFMA with z as the A operand - no partial sums through LDS;
//   * no __syncthreads anywhere.
// Same arithmetic as the multi-wave kernel per matrix element (same k-step order, same elimination), ref:LINE
// cites /root/reference/src/portfolio_calculations.py as there.
#include <utility>

#include "posterior_fused_impl.h"

namespace {

template <int NT_, bool LEAN_ = true>
struct WCfg {
    static constexpr int NT = NT_;
    static constexpr int KP = 16 * NT;
    static constexpr int NTILES = NT * (NT + 1) / 2;
    static constexpr int MLD = 17;                               // row stride of an M block (conflict-free both ways)
    static constexpr int OFF_M = 0;                              // [NT][16][MLD]  M_j = R_jj^-T, row-major
    static constexpr int OFF_DG = OFF_M + NT * 16 * MLD;         // [16][16] diagonal tile for the pivot chain, then two multiplier rows
    static constexpr int OFF_IDT = OFF_DG + 256;                 // [16][16] identity
    static constexpr int OFF_VEC = OFF_IDT + 256;                // [KP] column sums / Jeffreys t / y
    static constexpr int LDS_DOUBLES = OFF_VEC + KP;
    static constexpr int LDS_BYTES = LDS_DOUBLES * 8;
    // General (index) layout only, behind the fixed part: the panel rows of the pass in flight - and the daily pass's
    // per-row risk-free adjustments - staged in LDS once per pass: [rows] doubles, then [rows] ints, rows = wave_idx_rows().
    // Read from global memory inside the row loop they were a DEPENDENT load per k-step, and since s_waitcnt vmcnt counts
    // in order, waiting for the youngest load (the index) drained the whole three-k-step pipeline of row loads every step
    // (round 3: 30 % of the wave cycles of the index layout parked in s_waitcnt, 1.26 vs 1.04 ms at configs[1]).  LDS reads
    // are counted by lgkmcnt and are fetched one k-step ahead.  Sized per batch (dynamic LDS); batches whose passes would
    // not fit WAVE_LDS_LIMIT stay on the multi-wave kernel (wave_idx_fits).
    static constexpr int OFF_SUB = LDS_DOUBLES;
};
constexpr int WAVE_LDS_LIMIT = 64 * 1024;
// rows of the longest pass of a batch, rounded up to whole k-steps of 64 lanes' staging loads
__host__ __device__ inline int wave_idx_rows(int n_r, int m, bool conj) {
    const int r = (conj && m > n_r) ? m : n_r;
    return (r + 63) & ~63;
}
__host__ __device__ inline int wave_idx_bytes(int n_r, int m, bool conj) { return wave_idx_rows(n_r, m, conj) * 12; }

// row-major index of upper-triangle tile (I, J), I <= J - the numbering of the shared Gram tables
constexpr int wtile(int NT, int I, int J) { return I * NT - I * (I - 1) / 2 + (J - I); }

// Accumulator tile (I, J), I <= J, of a finished matrix into the kept posterior matrix P (k x k, row-major,
// tp_batch_keep_posterior; one- and two-wave kernels).  Register r of lane (fr, fq) holds element (16 I + fq + 4 r, 16 J + fr):
// the tile goes out as 128-byte row pieces (16 lanes), its mirror as 32-byte ones (the 4 lanes of a column fr).  Elements
// below the diagonal of a diagonal tile are not read: both halves of P come from the upper triangle, so P is exactly symmetric.
template <int I, int J>
__device__ __forceinline__ void wave_post_tile(double* P, int k, int fr, int fq, const d4& t) {
    const int gj = 16 * J + fr;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int gi = 16 * I + fq + 4 * r;
        if (gi < k && gj < k && (I < J || gi <= gj)) {
            tp_post_store(P + (long long)gi * k + gj, t[r]);
            if (I < J || gi < gj) tp_post_store(P + (long long)gj * k + gi, t[r]);
        }
    }
}

// ---- ownership: the upper triangle is split by tile COLUMN over the NWV waves of a window.  Tile column J belongs to wave
// w2_owner(J): snake over the columns from the widest (J = NT-1) down, so that every trailing sub-matrix of the
// factorisation stays balanced too.  The one-wave kernel is the case NWV = 1: one owner, every tile, numbered as wtile.
template <int NT, int NWV>
constexpr int w2_owner(int J) {
    const int p = NT - 1 - J, g = p / NWV, i = p % NWV;
    return (g & 1) ? NWV - 1 - i : i;
}
template <int NT, int NWV>
constexpr int w2_count(int WV) {
    int n = 0;
    for (int J = 0; J < NT; ++J)
        if (w2_owner<NT, NWV>(J) == WV) n += J + 1;
    return n;
}
template <int NT, int NWV>
constexpr int w2_max_tiles() {
    int m = 0;
    for (int w = 0; w < NWV; ++w) m = w2_count<NT, NWV>(w) > m ? w2_count<NT, NWV>(w) : m;
    return m;
}
// slot of tile (I, J) among its owner's tiles (row-major over the owner's tiles); -1 when I > J
template <int NT, int NWV>
constexpr int w2_slot(int I, int J) {
    const int wv = w2_owner<NT, NWV>(J);
    int n = 0;
    for (int i = 0; i < NT; ++i)
        for (int j = i; j < NT; ++j) {
            if (i == I && j == J) return n;
            if (w2_owner<NT, NWV>(j) == wv) ++n;
        }
    return -1;
}
// does wave WV own any tile column J >= I (i.e. does it need the A operand of tile row I in a trailing update)?
template <int NT, int NWV>
constexpr bool w2_owns_from(int WV, int I) {
    for (int J = I; J < NT; ++J)
        if (w2_owner<NT, NWV>(J) == WV) return true;
    return false;
}
// NWV = 1 is the one-wave kernel's numbering, for every tile count built
template <int NT>
constexpr bool w2_one_wave_is_whole() {
    for (int J = 0; J < NT; ++J) {
        if (w2_owner<NT, 1>(J) != 0) return false;
        for (int I = 0; I <= J; ++I)
            if (w2_slot<NT, 1>(I, J) != wtile(NT, I, J)) return false;
    }
    return w2_count<NT, 1>(0) == NT * (NT + 1) / 2;
}
template <int... N>
constexpr bool w2_one_wave_is_whole_all(std::integer_sequence<int, N...>) { return (w2_one_wave_is_whole<N + 1>() && ...); }
static_assert(w2_one_wave_is_whole_all(std::make_integer_sequence<int, 15>{}),
              "w2_owner<NT,1>(J) == 0, w2_slot<NT,1>(I,J) == wtile(NT,I,J), w2_count<NT,1>(0) == NT(NT+1)/2 for NT = 1..15");

// The MFMAs of the Gram loops are inline assembly, which the compiler's hazard recogniser does not see: a
// v_mfma_f64_16x16x4 result may be read by anything but the SrcC of the next MFMA on the same registers only 19
// wait states after issue (what hipcc inserts behind the builtin).  Every pass over rows ends in a settle; the asm
// "modifies" every tile, so no later use of an accumulator can be scheduled in front of the wait.
// Where a tile lives.  The first 32 tiles fill the AGPR half of the register file (256 registers); tile counts of 8 and
// 9 per side (36 / 45 tiles) keep the rest in VGPRs - MFMA accumulators may be either.
constexpr bool wave_tile_in_agpr(int t) { return t < 32; }

// s_nop 1: a VGPR written by a vector instruction may be read as an MFMA operand two wait states later at the earliest
// (hipcc puts the same s_nop in front of the builtin); the asm carries it because the compiler cannot see the hazard.
template <int T>
__device__ __forceinline__ void wave_mfma_agpr(d4& c, double a, double b) {
    if constexpr (wave_tile_in_agpr(T)) asm volatile("s_nop 1\n\tv_mfma_f64_16x16x4_f64 %0, %1, %2, %0" : "+a"(c) : "v"(a), "v"(b));
    else asm volatile("s_nop 1\n\tv_mfma_f64_16x16x4_f64 %0, %1, %2, %0" : "+v"(c) : "v"(a), "v"(b));
}
template <int T>
__device__ __forceinline__ void wave_settle1(d4& c0) {
    if constexpr (wave_tile_in_agpr(T)) asm volatile("s_nop 15\n\ts_nop 7" : "+a"(c0));
    else asm volatile("s_nop 15\n\ts_nop 7" : "+v"(c0));
}
// Entering a row loop: hand the loop-carried accumulators over as AGPR values (an empty asm that "modifies" them), so
// that the loop's phi nodes become AGPR phis; otherwise the accumulators live in VGPRs across the back edge and are
// copied into AGPRs for the asm MFMAs on every iteration.
template <int T>
__device__ __forceinline__ void wave_pin1(d4& c0) {
    if constexpr (wave_tile_in_agpr(T)) asm volatile("" : "+a"(c0));
    else asm volatile("" : "+v"(c0));
}
__device__ __forceinline__ void wave_settle14(d4& c0, d4& c1, d4& c2, d4& c3, d4& c4, d4& c5, d4& c6, d4& c7, d4& c8, d4& c9,
                                              d4& c10, d4& c11, d4& c12, d4& c13) {
    asm volatile("s_nop 15\n\ts_nop 7" : "+a"(c0), "+a"(c1), "+a"(c2), "+a"(c3), "+a"(c4), "+a"(c5), "+a"(c6), "+a"(c7), "+a"(c8),
                 "+a"(c9), "+a"(c10), "+a"(c11), "+a"(c12), "+a"(c13));
}
// entering a row loop: every loop-carried accumulator as an AGPR (tiles >= 32: VGPR) value - wave_pin1
template <int N>
__device__ __forceinline__ void wave_pin(d4 (&acc)[N]) {
    static_for<0, N>([&](auto tc) __attribute__((always_inline)) { wave_pin1<decltype(tc)::value>(acc[decltype(tc)::value]); });
}
// End of a pass of inline-assembly MFMAs.  GROUPED (the one-wave kernel): one wait per group of 14 tiles.  Otherwise (the
// two- / four-wave kernel): 24 wait states once, then every tile is "modified" behind them (asm volatile statements keep
// their order).  The two emit different instructions; each kernel keeps the form it was tuned and hazard-checked with.
template <bool GROUPED, int N>
__device__ __forceinline__ void wave_settle(d4 (&acc)[N]) {
    if constexpr (GROUPED) {
        static_for<0, (N + 13) / 14>([&](auto gc) __attribute__((always_inline)) {
            constexpr int b = 14 * decltype(gc)::value;
            if constexpr (b + 14 <= N && wave_tile_in_agpr(b + 13)) {
                wave_settle14(acc[b], acc[b + 1], acc[b + 2], acc[b + 3], acc[b + 4], acc[b + 5], acc[b + 6], acc[b + 7], acc[b + 8],
                              acc[b + 9], acc[b + 10], acc[b + 11], acc[b + 12], acc[b + 13]);
            } else {
                static_for<b, (b + 14 < N ? b + 14 : N)>([&](auto tc) __attribute__((always_inline)) {
                    wave_settle1<decltype(tc)::value>(acc[decltype(tc)::value]);
                });
            }
        });
    } else {
        wave_settle1<0>(acc[0]);
        static_for<1, N>([&](auto tc) __attribute__((always_inline)) { wave_pin1<decltype(tc)::value>(acc[decltype(tc)::value]); });
    }
}

// ---- accumulators STARTED from a table slot (the PRE form of the one-wave kernel, wave_window_body).  A slot is
// [tile][2][64 lanes][2] doubles - the accumulator layout - so tile T is two 16-byte loads per lane, and a global load may
// name AGPRs as its destination: no VGPR visit, no add.  The two loads fill the halves of ONE eight-register operand, which
// inline assembly can only say with the registers' names: tile T of the AGPR-resident tiles is loaded into a[8T:8T+7]
// (a physical-register output).  The allocator keeps the value there (checked on the ISA: no v_accvgpr move follows).
// The compiler counts neither load: wave_slot_arrive1 - s_waitcnt vmcnt(0), which "modifies" the tile - stands between
// the load and every use, and tools/check_mfma_hazards.py proves on the ISA that nothing touches a destination in between.
// Address: lane-uniform slot base + 2048 T in SGPRs (scalar adds), 16 lane in one VGPR.
template <int T>
__device__ __forceinline__ void wave_slot_load(d4& c, const double* slot_tile, unsigned lane16);
#define TP_SLOT_LOAD(T, R0, R3, R4, R7)                                                                                        \
    template <>                                                                                                                 \
    __device__ __forceinline__ void wave_slot_load<T>(d4& c, const double* slot_tile, unsigned lane16) {                        \
        asm volatile("global_load_dwordx4 a[" #R0 ":" #R3 "], %1, %2\n\tglobal_load_dwordx4 a[" #R4 ":" #R7 "], %1, %2 offset:1024" \
                     : "={a[" #R0 ":" #R7 "]}"(c)                                                                               \
                     : "v"(lane16), "s"(slot_tile)                                                                              \
                     : "memory");                                                                                               \
    }
TP_SLOT_LOAD(0, 0, 3, 4, 7) TP_SLOT_LOAD(1, 8, 11, 12, 15) TP_SLOT_LOAD(2, 16, 19, 20, 23) TP_SLOT_LOAD(3, 24, 27, 28, 31)
TP_SLOT_LOAD(4, 32, 35, 36, 39) TP_SLOT_LOAD(5, 40, 43, 44, 47) TP_SLOT_LOAD(6, 48, 51, 52, 55) TP_SLOT_LOAD(7, 56, 59, 60, 63)
TP_SLOT_LOAD(8, 64, 67, 68, 71) TP_SLOT_LOAD(9, 72, 75, 76, 79) TP_SLOT_LOAD(10, 80, 83, 84, 87) TP_SLOT_LOAD(11, 88, 91, 92, 95)
TP_SLOT_LOAD(12, 96, 99, 100, 103) TP_SLOT_LOAD(13, 104, 107, 108, 111) TP_SLOT_LOAD(14, 112, 115, 116, 119)
TP_SLOT_LOAD(15, 120, 123, 124, 127) TP_SLOT_LOAD(16, 128, 131, 132, 135) TP_SLOT_LOAD(17, 136, 139, 140, 143)
TP_SLOT_LOAD(18, 144, 147, 148, 151) TP_SLOT_LOAD(19, 152, 155, 156, 159) TP_SLOT_LOAD(20, 160, 163, 164, 167)
TP_SLOT_LOAD(21, 168, 171, 172, 175) TP_SLOT_LOAD(22, 176, 179, 180, 183) TP_SLOT_LOAD(23, 184, 187, 188, 191)
TP_SLOT_LOAD(24, 192, 195, 196, 199) TP_SLOT_LOAD(25, 200, 203, 204, 207) TP_SLOT_LOAD(26, 208, 211, 212, 215)
TP_SLOT_LOAD(27, 216, 219, 220, 223) TP_SLOT_LOAD(28, 224, 227, 228, 231) TP_SLOT_LOAD(29, 232, 235, 236, 239)
TP_SLOT_LOAD(30, 240, 243, 244, 247) TP_SLOT_LOAD(31, 248, 251, 252, 255)
#undef TP_SLOT_LOAD
template <int T>
__device__ __forceinline__ void wave_slot_arrive1(d4& c) {
    static_assert(wave_tile_in_agpr(T), "VGPR-resident tiles are loaded by the compiler's own (counted) loads");
    asm volatile("s_waitcnt vmcnt(0)" : "+a"(c));
}
// every tile of a window from the slot at `q`: the AGPR-resident tiles as above, the VGPR-resident ones (tiles 32.., eight
// and nine tiles per side) by plain loads, which the compiler counts and waits for itself
template <int N>
__device__ __forceinline__ void wave_slot_issue(d4 (&acc)[N], const double* q, int lane) {
    typedef double d2 __attribute__((ext_vector_type(2)));
    const unsigned lane16 = 16u * (unsigned)lane;
    static_for<0, N>([&](auto tc) __attribute__((always_inline)) {
        constexpr int t = decltype(tc)::value;
        if constexpr (wave_tile_in_agpr(t)) {
            wave_slot_load<t>(acc[t], q + 256 * t, lane16);
        } else {
            const d2* p = (const d2*)(q + 256 * t) + lane;
            const d2 lo = p[0], hi = p[64];
            acc[t] = d4{lo[0], lo[1], hi[0], hi[1]};
        }
    });
}
template <int N>
__device__ __forceinline__ void wave_slot_arrive(d4 (&acc)[N]) {
    static_for<0, N>([&](auto tc) __attribute__((always_inline)) {
        constexpr int t = decltype(tc)::value;
        if constexpr (wave_tile_in_agpr(t)) wave_slot_arrive1<t>(acc[t]);
        else wave_pin1<t>(acc[t]);
    });
}

struct WRows {
    const double* base;     // panel
    long long ld;           // leading dimension (doubles)
    const int* ridx;        // explicit rows of this window, or nullptr
    long long first;        // first row (contiguous)
    const double* sub_row;  // per-row subtrahend (rf_adj) or nullptr
    int count;              // rows
    int count0;             // contiguous, two row ranges: staged rows r >= count0 are panel rows first + r + jump
    int jump;
    bool off32 = false;     // general layout: row * 8 ld + 8 column fits 32 bits for every row of the PANEL (host-checked)
};

// One pass over the rows of a window for wave WV of NWV: acc(I,J) += rows[:, I]' rows[:, J] for the tile columns J it owns,
// 4 rows per k-step.
//  HF:   intraday rows, shifted by `shift` (the window's first row, or its column means), column k carries
//        u_r = (y_r - shift).w0 and - when `ones` - column k+1 carries ones (one-pass centring, phase C)
//  !HF:  daily rows minus the per-row risk-free adjustment, column k carries ones (t = X'1, ref:222)
//  lazy_mask (HF): `shift` and `w0v` arrive as RAW loads (padding columns hold column k-1's values); they are zeroed
//  beyond column k here, AFTER the first two k-steps' row loads have been issued - masking them at the call site made the
//  wave wait for the shift row before it could ask for the first panel rows (two memory round trips in a row, and this
//  wave has nothing else to run meanwhile)
//  !LEAN: lds_rows[r] / lds_sub[r] hold the panel row and the subtrahend of row r of this pass (staged by wave_stage_rows)
//  PRE (one-wave kernel, HF, LEAN, ones; defaults to off - every other caller compiles to what it was): the accumulators
//  arrive UNDEFINED and start as the table slot at `slot`, loaded behind the first two k-steps' row loads; the shifted rows
//  are scaled by `rsc` (subtract, then multiply: a constant column stays exactly zero), column k stays zero (it holds the
//  slot's t) and u_r goes to column k+2
//  TROW (one-wave kernel, !HF, LEAN: the preloaded form's edge rows; defaults to off - every other caller compiles to what it
//  was): ONE more row behind the last, with DIFFERENT operands on the two sides - acc(I,J) += ta[I] tb[J] in row slot
//  src.count (the centring's rank-one term, wave_window_body).  The pass is src.count + 1 slots long, so that slot is always
//  in the LAST k-step, which is always one of the (at most three) k-steps behind the main loop; `ta` / `tb` arrive non-zero
//  only in the lanes of that slot (fq == src.count & 3).  Those k-steps take their masked-out lanes from ta / tb instead of
//  zero: nothing in the k-steps in front of the last (every lane holds a row), the row and zeros behind it in the last.  When
//  src.count = 0 (mod 4) - zero rows included - the row has a k-step of its own.  Its load re-reads the last row (row 0 of
//  the window when there is none), as the padding slots do.
template <int NT, int NWV, int WV, bool HF, bool LEAN, bool PRE = false, bool TROW = false>
__device__ __forceinline__ void wave_gram(const WRows& src, const long long (&coff)[NT], int k, int lane,
                                          double (&shift)[NT], double (&w0v)[NT], bool ones, bool lazy_mask,
                                          d4 (&acc)[w2_count<NT, NWV>(WV)], const int* lds_rows, const double* lds_sub,
                                          double (&csum)[NT], double& usum, double rsc = 1.0, const double* slot = nullptr,
                                          const double* ta = nullptr, const double* tb = nullptr) {
    static_assert(!PRE || (HF && LEAN && NWV == 1), "the preloaded form exists for the one-wave kernel's intraday pass only");
    static_assert(!TROW || (!HF && LEAN && NWV == 1 && !PRE), "the trailing row exists for the preloaded form's edge rows only");
    constexpr int kI = NT - 1;
    const int fr = lane & 15, fq = lane >> 4;
    const int kc = k - 16 * kI;
    const bool cvl = fr < kc;
    const double border = HF ? ((ones && fr == kc + 1) ? 1.0 : 0.0) : ((fr == kc) ? 1.0 : 0.0);
    const int nks = (src.count + (TROW ? 1 : 0) + 3) >> 2;
    const bool has_sub = !HF && src.sub_row != nullptr;

    // general layout: the pass's panel rows (and subtrahends) come from LDS; the values of the NEXT load are fetched right
    // behind the current load's requests, a whole k-step of MFMAs ahead of their use
    int row_pref = 0;
    double sub_pref = 0.0;
    auto prefetch = [&](int ks) __attribute__((always_inline)) {
        int r = 4 * ks + fq;
        r = r < src.count ? r : src.count - 1;
        row_pref = lds_rows[r];
        if (has_sub) sub_pref = lds_sub[r];
    };
    if constexpr (!LEAN) prefetch(0);
    // 32-bit addressing: a wave-uniform 64-bit base (the window's first row; general layout: the panel) + row * (8 ld) +
    // 8 column, ONE 24-bit multiply-add per operand (the 64-bit row * ld product cost 15 vector instructions per k-step).
    // The contiguous layout always qualifies (tp_layout_is_lean); the general layout when the panel is below 4 GiB
    // (tp_kargs_t::panel_off32 / hf_off32 bit 0), else it keeps 64-bit addresses.
    const char* ub = (const char*)(LEAN ? src.base + src.first * src.ld : src.base);
    const unsigned ld8 = (unsigned)src.ld * 8u;
    unsigned c8[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i) c8[i] = 8u * (unsigned)coff[i];
    auto load = [&](double (&v)[NT], double& sub, int ks) __attribute__((always_inline)) {
        int r = 4 * ks + fq;
        r = r < src.count ? r : src.count - 1;                      // rows past the end re-read the last row (masked below)
        if constexpr (TROW) r = r < 0 ? 0 : r;                      // (no row at all: row 0 of the window)
        if (LEAN || src.off32) {
            unsigned row;
            if constexpr (LEAN) row = (unsigned)(r + (r >= src.count0 ? src.jump : 0));
            else row = (unsigned)row_pref;
            if constexpr (LEAN) {
                // ungathered columns: group i sits 128 i bytes behind group 0 (immediate offsets); only the last group clamps
                const unsigned r0 = __umul24(row, ld8) + c8[0];
#pragma unroll
                for (int i = 0; i < NT - 1; ++i) v[i] = *(const double*)(ub + (size_t)r0 + 128 * i);
                v[NT - 1] = *(const double*)(ub + (size_t)(__umul24(row, ld8) + c8[NT - 1]));
            } else {
                const unsigned ro = __umul24(row, ld8);
#pragma unroll
                for (int i = 0; i < NT; ++i) v[i] = *(const double*)(ub + (size_t)(ro + c8[i]));
            }
        } else {
            const double* p = src.base + (long long)row_pref * src.ld;
#pragma unroll
            for (int i = 0; i < NT; ++i) v[i] = p[coff[i]];
        }
        sub = 0.0;
        if constexpr (!LEAN) {
            if (has_sub) sub = sub_pref;
            prefetch(ks + 1);                                       // loads are issued for ks = 0, 1, 2, ... in this order
        } else {
            if (has_sub) sub = src.sub_row[r];                       // contiguous rows with a risk-free adjustment (rare)
        }
    };
    // MASK: the k-step may hold rows past the end (only the last three k-steps of a pass are built with it)
    auto step = [&](double (&v)[NT], double sub, int ks, auto maskc) __attribute__((always_inline)) {
        constexpr bool MASK = decltype(maskc)::value != 0;
        if (HF) {
#pragma unroll
            for (int i = 0; i < NT; ++i) v[i] -= shift[i];
            if constexpr (PRE) {
#pragma unroll
                for (int i = 0; i < NT; ++i) v[i] *= rsc;
            }
        } else if (has_sub) {
#pragma unroll
            for (int i = 0; i < NT; ++i) v[i] -= sub;                // ref:57
        }
        v[kI] = cvl ? v[kI] : border;
        if (MASK) {
            const bool rv = 4 * ks + fq < src.count;
#pragma unroll
            for (int i = 0; i < NT; ++i) v[i] = rv ? v[i] : 0.0;
        }
        if (HF) {
            double z = 0.0;
#pragma unroll
            for (int i = 0; i < NT; ++i) z = fma(v[i], w0v[i], z);
            z = rowgroup_sum16(z);
            if (!ones) {
                // k + 1 = 0 (mod 16): no spare column for the ones of the one-pass centring - the column sums of the
                // shifted rows (and the sum of u) are kept by vector adds instead: NT + 1 per k-step next to the MFMAs
                // (round 2 ran a separate pass for the column MEANS at these sizes: a second dependent trip to memory,
                // 13.8 % of a window's time at k = 191)
#pragma unroll
                for (int i = 0; i < NT; ++i) csum[i] += v[i];
                usum += z;
            }
            if (fr == (PRE ? kc + 2 : kc)) v[kI] = z;                // u_r = (y_r - shift).w0
        }
        static_for<0, NT>([&](auto Ic) __attribute__((always_inline)) {
            constexpr int I = decltype(Ic)::value;
            static_for<I, NT>([&](auto Jc) __attribute__((always_inline)) {
                constexpr int J = decltype(Jc)::value;
                if constexpr (w2_owner<NT, NWV>(J) == WV) {
                    constexpr int t = w2_slot<NT, NWV>(I, J);
                    // accumulators pinned to the AGPR half of the register file: left to itself the allocator moved the
                    // whole accumulator set between VGPRs and AGPRs inside this loop (497 v_accvgpr moves per 84 MFMAs)
                    wave_mfma_agpr<t>(acc[t], v[I], v[J]);
                }
            });
        });
    };
    // TROW: a k-step behind the main loop - lanes without a row take ta (A side) and tb (B side) in place of zero
    [[maybe_unused]] auto step_t = [&](double (&v)[NT], double sub, int ks) __attribute__((always_inline)) {
        if (has_sub) {
#pragma unroll
            for (int i = 0; i < NT; ++i) v[i] -= sub;
        }
        v[kI] = cvl ? v[kI] : border;
        const bool rv = 4 * ks + fq < src.count;
        double vt[NT];
#pragma unroll
        for (int i = 0; i < NT; ++i) {
            vt[i] = rv ? v[i] : tb[i];
            v[i] = rv ? v[i] : ta[i];
        }
        static_for<0, NT>([&](auto Ic) __attribute__((always_inline)) {
            constexpr int I = decltype(Ic)::value;
            static_for<I, NT>([&](auto Jc) __attribute__((always_inline)) {
                constexpr int J = decltype(Jc)::value;
                constexpr int t = w2_slot<NT, NWV>(I, J);
                wave_mfma_agpr<t>(acc[t], v[I], vt[J]);
            });
        });
    };

    if constexpr (!PRE) {
        if (nks <= 0) return;
    }
    // Three register sets rotate through load -> (two k-steps of MFMAs) -> use.  The main loop runs whole triples of
    // full k-steps as ONE basic block (loads past the end re-read the last row); at most three k-steps remain.
    double va[NT], vb[NT], vc[NT];
    double sa = 0.0, sb = 0.0, sc = 0.0;
    load(va, sa, 0);
    load(vb, sb, 1);
    if constexpr (PRE) {
        __builtin_amdgcn_sched_barrier(0);
        wave_slot_issue(acc, slot, lane);
    }
    if (HF && lazy_mask) {
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < NT; ++i) {
            const bool cv = 16 * i + fr < k;
            shift[i] = cv ? shift[i] : 0.0;
            w0v[i] = cv ? w0v[i] : 0.0;
        }
    }
    if constexpr (PRE) wave_slot_arrive(acc);
    else wave_pin(acc);
    int ks = 0;
#pragma nounroll
    for (; 4 * (ks + 3) <= src.count; ks += 3) {
        load(vc, sc, ks + 2);
        step(va, sa, ks, ic<0>{});
        load(va, sa, ks + 3);
        step(vb, sb, ks + 1, ic<0>{});
        load(vb, sb, ks + 4);
        step(vc, sc, ks + 2, ic<0>{});
    }
    if constexpr (TROW) {
        if (ks + 2 < nks) load(vc, sc, ks + 2);
        step_t(va, sa, ks);
        if (ks + 1 < nks) step_t(vb, sb, ks + 1);
        if (ks + 2 < nks) step_t(vc, sc, ks + 2);
    } else if (ks < nks) {
        if (ks + 2 < nks) load(vc, sc, ks + 2);
        step(va, sa, ks, ic<1>{});
        if (ks + 1 < nks) step(vb, sb, ks + 1, ic<1>{});
        if (ks + 2 < nks) step(vc, sc, ks + 2, ic<1>{});
    }
    wave_settle<NWV == 1>(acc);
}

// General layout: panel row (and subtrahend) of every row of the pass into LDS, 64 rows per instruction.
__device__ __forceinline__ void wave_stage_rows(const WRows& src, int lane, int* li, double* lsb) {
    for (int i = lane; i < src.count; i += 64) {
        li[i] = src.ridx ? src.ridx[i] : (int)(src.first + i);
        if (src.sub_row) lsb[i] = src.sub_row[i];
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// Phases A-E below are written out here AND in w2_body (posterior_wave2_impl.h) with its ownership filter: each of these
// pieces, moved into a function of its own, changed the instruction stream of some kernel (DESIGN.md section 4f,
// profiles/r07_wave_kernels_refactor_isa.txt); they keep this source form until such a change has been timed.
// MODE 3 / 4: MODE 0 / 1 plus the store of the posterior matrix (tp_batch_keep_posterior) - instantiations of their own, so
// that the plain modes' code is exactly what it was without the feature.
// MODE 0: conjugate, 1: Jeffreys - the plain product paths, compiled without the read-back / custom right-hand side /
// shift branches: every branch that merges two versions of the accumulators costs register copies or spills here (one
// kernel with all of them decided at run time, MODE 2, needs 2.2 KB of scratch per lane against 44 bytes, and spill code
// next to the inline-assembly MFMAs is exactly what the hazard argument of wave_settle cannot cover).  MODE 2 is therefore
// not instantiated: batches that ask for a matrix read-back, a custom right-hand side, tp_batch_keep_rhs or a shift run
// on the multi-wave kernel (wave_mode / launch_one).
// PRE (plain conjugate, LEAN, a batch with shared tables, kc <= 13; wave_launch_variant decides): the accumulators START as
// the window's table slot Q_L[b0] (wave_gram, PRE), the intraday rows are accumulated on top of it already scaled by
// sqrt(sc), and the rank-one term of the centring is ONE row behind the last daily edge row, in that pass's last k-step
// (wave_gram, TROW): between the row loops only the term's operands are read out of tile column kI (phase C), and the border
// pass over that tile column (q0, c, column k += c column k+2) follows the edge rows - no pass over all tiles and no table
// addition.  Columns: k the slot's t, k+1 ones, k+2 u.  Windows of such a batch without a slot of their own start from the
// tables' all-zero slot.
template <int NT, bool LEAN, int MODE, bool PRE = false>
__device__ __forceinline__ void wave_window_body(const tp_kargs_t& A, double* lds) {
    static_assert(!PRE || (LEAN && (MODE == 0 || MODE == 3)), "preloaded accumulators: plain conjugate, contiguous layout");
    constexpr bool FULL = MODE == 2;
    constexpr bool POST = MODE >= 3;
    constexpr int PLAIN = POST ? MODE - 3 : MODE;
    using C = WCfg<NT, LEAN>;
    const int lane = threadIdx.x;
    const int fr = lane & 15, fq = lane >> 4;
    const int k = A.k;
    __builtin_assume(k >= 16 * (NT - 1));
    __builtin_assume(k <= 16 * NT - 1);
    constexpr int kI = NT - 1;
    const int kc = k - 16 * kI;
    const int NTB = (kc == 0) ? NT - 1 : NT;
    const bool colv = fr < kc;
    // XCD-aware workgroup -> window map (see posterior_fused_impl.h): one contiguous window range per XCD
    const long long per_xcd = (A.w_count + 7) >> 3;
    const long long wl = (long long)(blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3);
    if ((long long)(blockIdx.x >> 3) >= per_xcd || wl >= A.w_count) return;
    const long long w = A.w_first + wl;
    const int tid0 = lane;
    (void)tid0;

    const int* cols = (!LEAN && A.col_idx) ? A.col_idx + w * k : nullptr;
    // column offsets (doubles) of this lane in the NT column groups, once per window; padding columns re-read column k-1.
    // The gathered columns' indices are requested together (one wait), not one dependent load per select.
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
    // general layout: staging region of the pass in flight behind the fixed part of the LDS image
    double* idx_sub_lds = LEAN ? nullptr : lds + C::OFF_SUB;
    int* idx_rows_lds = LEAN ? nullptr : (int*)(lds + C::OFF_SUB + wave_idx_rows(A.n_r, A.m, A.strategy == 0));
    d4 acc[C::NTILES];
    if constexpr (!PRE) {
    static_for<0, C::NTILES>([&](auto tc) __attribute__((always_inline)) { acc[decltype(tc)::value] = d4{0.0, 0.0, 0.0, 0.0}; });
    // AGPR values from the first definition on: where two paths of the kernel meet, the accumulators must arrive as AGPR
    // values on both, or the merge keeps all of them in VGPRs (and spills)
    wave_pin(acc);
    }

    // identity tile for the pivot chain (read after many waits on this wave's own LDS traffic)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int e = lane + 64 * i;
        lds[C::OFF_IDT + e] = ((e >> 4) == (e & 15)) ? 1.0 : 0.0;
    }

    double n0 = 0.0, cc = 0.0, q0 = 0.0;
    const bool conj = PLAIN == 0 ? true : PLAIN == 1 ? false : (A.strategy == 0);
    const int dbg = (FULL && A.dbg_S1 != nullptr && w == A.dbg_w) ? A.dbg_mode : 0;

    auto dump_matrix = [&]() __attribute__((always_inline)) {
        static_for<0, NT>([&](auto Ic) __attribute__((always_inline)) {
            constexpr int I = decltype(Ic)::value;
            static_for<I, NT>([&](auto Jc) __attribute__((always_inline)) {
                constexpr int J = decltype(Jc)::value;
                constexpr int t = wtile(NT, I, J);
                const int gj = 16 * J + fr;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int gi = 16 * I + fq + 4 * r;
                    if (gi < k && gj < k) {
                        A.dbg_S1[(long long)gi * k + gj] = acc[t][r];
                        A.dbg_S1[(long long)gj * k + gi] = acc[t][r];
                    }
                    if (gi < k && gj == k) A.dbg_S1[(long long)k * k + gi] = acc[t][r];
                }
            });
        });
    };
    // value of element (row kc, column kc) of tile (kI, kI): the corner of the bordered matrix.  All four registers are
    // read and the SCALAR results selected: a run-time choice among the four vector registers came out of hipcc as a
    // branch ladder that left the value undefined for kc >= 12 in some instantiations (k = 31, 63: garbage q0).
    auto corner = [&]() __attribute__((always_inline)) {
        constexpr int t = wtile(NT, kI, kI);
        const int ln = __builtin_amdgcn_readfirstlane(16 * (kc & 3) + kc);
        const double x0 = readlane_d(acc[t][0], ln), x1 = readlane_d(acc[t][1], ln);
        const double x2 = readlane_d(acc[t][2], ln), x3 = readlane_d(acc[t][3], ln);
        const int rr = kc >> 2;
        return rr == 0 ? x0 : rr == 1 ? x1 : rr == 2 ? x2 : x3;
    };

    TP_MARK(0);
    if constexpr (PRE) {
        n0 = A.n0[w];
        WRows hs;
        hs.base = A.hf_panel; hs.ld = A.hf_ld;
        hs.ridx = nullptr;
        hs.first = A.hf_start ? A.hf_start[w] : 0;
        hs.sub_row = nullptr;
        hs.count = A.hf_count ? A.hf_count[w] : A.m;
        hs.count0 = 0x7fffffff; hs.jump = 0;
        hs.off32 = (A.hf_off32 & 1) != 0;
        // the daily window first: its table slot is what the accumulators start from (phase D: the edge rows alone)
        WRows ds;
        ds.base = A.panel; ds.ld = A.panel_ld;
        ds.ridx = nullptr;
        ds.first = A.start ? A.start[w] : 0;
        ds.sub_row = nullptr;                                       // (a batch with rf_adj has no tables)
        ds.count = A.n_rows ? A.n_rows[w] : A.n_r;
        ds.count0 = 0x7fffffff; ds.jump = 0;
        ds.off32 = (A.panel_off32 & 1) != 0;
        const double* q;
        {
            constexpr int BLK = 16;
            const long long b0 = (ds.first + BLK - 1) / BLK, b1 = (ds.first + ds.count) / BLK;
            const int Lw = (int)(b1 - b0);
            const int li = Lw == A.winsum_L[0] ? 0 : Lw == A.winsum_L[1] ? 1 : Lw == A.winsum_L[2] ? 2 : Lw == A.winsum_L[3] ? 3 : -1;
            const bool shared = Lw > 0 && li >= 0;
            // no branch around the loads: a window without a slot of its own reads the all-zero slot, and every row of it
            // goes through the MFMAs
            const int c0 = (int)(BLK * b0 - ds.first);
            ds.count0 = shared ? c0 : 0x7fffffff;
            ds.jump = shared ? (int)(BLK * b1 - ds.first) - c0 : 0;
            ds.count = shared ? c0 + (int)(ds.first + ds.count - BLK * b1) : ds.count;
            // no edge row at all: the centring row's load re-reads row 0 of the window, not the row behind its last block
            ds.count0 = ds.count > 0 ? ds.count0 : 0x7fffffff;
            q = shared ? A.winsum + ((long long)li * A.prefix_nblk + b0) * ((long long)C::NTILES * 256) : A.winsum_zero;
        }
        // ---- phase A: the shift row (the window's first intraday row), w0
        double shift[NT], w0v[NT], csum[NT];
        double usum = 0.0;
        {
            const double* p0 = hs.base + hs.first * (long long)hs.ld;
#pragma unroll
            for (int i = 0; i < NT; ++i) {
                const int c = 16 * i + fr;
                const int cl = c < k ? c : k - 1;
                shift[i] = p0[coff[i]];      // raw: zeroed beyond column k inside wave_gram (lazy_mask)
                w0v[i] = A.w0[w * k + cl];
                csum[i] = 0.0;
            }
        }
        const double mm = (double)hs.count;
        const double invm = 1.0 / mm;
        const double rsc = sqrt(n0 * (mm / (mm - 1.0)));           // rows scaled by sqrt(sc): the Gram accumulates S0 = sc C
        TP_MARK(1);
        // ---- phase B: slot + Gram of the scaled shifted intraday rows (from row 1: the shift row itself is zero)
        hs.first += 1; hs.count -= 1;
        wave_gram<NT, 1, 0, true, true, true>(hs, coff, k, lane, shift, w0v, true, true, acc, nullptr, nullptr, csum, usum, rsc, q);
        TP_MARK(2);
        // ---- phase C: tau, the operands of the centring's rank-one term acc(I,J) += (-tau_I / m) tau_J, handed over through
        // OFF_VEC.  tau = column k+1 (sqrt(sc) sums of the shifted rows) over the asset rows, zero at k and k+1, and at k+2 the
        // sum of u - element (k+1, k+2).  The term itself rides in the edge rows' last k-step (wave_gram, TROW): the edge rows
        // are zero at k+1 and k+2 and tau is zero at k and k+1, so the two touch no common element but the asset block, where
        // they only add.  Behind phase D column k+2 is sc C w0 and element (k+2, k+2) is q0.
        static_for<0, NT>([&](auto Ic) __attribute__((always_inline)) {
            constexpr int I = decltype(Ic)::value;
            constexpr int t = wtile(NT, I, kI);
            if (fr == kc + 1) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = fq + 4 * r;
                    if (I < kI) lds[C::OFF_VEC + 16 * I + row] = acc[t][r];
                    else if (row != kc + 2) lds[C::OFF_VEC + 16 * I + row] = row < kc ? acc[t][r] : 0.0;
                }
            }
            if (I == kI && fr == kc + 2) {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (fq + 4 * r == kc + 1) lds[C::OFF_VEC + 16 * I + kc + 2] = acc[t][r];
            }
        });
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        // the row slot behind the last edge row: slot ds.count, lanes fq == ds.count & 3 of the pass's last k-step
        double ta[NT], tb[NT];
        {
            const int tq = ds.count & 3;
#pragma unroll
            for (int J = 0; J < NT; ++J) {
                const double tv = lds[C::OFF_VEC + 16 * J + fr];
                tb[J] = fq == tq ? tv : 0.0;
                ta[J] = fq == tq ? -(tv * invm) : 0.0;
            }
        }
        TP_MARK(3);
        // ---- phase D: the daily edge rows (ref:180), ones in the border column (t, ref:222), and the centring row behind
        // them; the whole blocks came with the slot
        TP_MARK(32);
        double none[NT] = {};
        double nosum = 0.0;
        wave_gram<NT, 1, 0, false, true, false, true>(ds, coff, k, lane, none, none, false, false, acc, nullptr, nullptr, none, nosum,
                                                      1.0, nullptr, ta, tb);
        TP_MARK(33);
        // scalars (ref:415-418): q0 = w0'S0 w0 is the element (k+2, k+2) - all four registers read, see `corner`
        {
            constexpr int t = wtile(NT, kI, kI);
            const int kx = kc + 2;
            const int ln = __builtin_amdgcn_readfirstlane(16 * (kx & 3) + kx);
            const double x0 = readlane_d(acc[t][0], ln), x1 = readlane_d(acc[t][1], ln);
            const double x2 = readlane_d(acc[t][2], ln), x3 = readlane_d(acc[t][3], ln);
            const int rr = kx >> 2;
            q0 = rr == 0 ? x0 : rr == 1 ? x1 : rr == 2 ? x2 : x3;
        }
        // (k through an opaque scalar copy: merged with phase H's own conversion of k, the double lived in a VGPR pair across
        // the whole factorisation - and was spilled, 12 bytes of scratch at seven tiles per side)
        int kq = k;
        asm("" : "+s"(kq));
        const double a = n0 + kq + 2;
        cc = (2 * n0) / (a + sqrt(a * a + 4 * n0 * q0));
        // border pass, tile column kI only: column k (the slot's t) += c * column k+2 (two lanes up in the row group),
        // columns beyond k cleared
        static_for<0, NT>([&](auto Ic) __attribute__((always_inline)) {
            constexpr int I = decltype(Ic)::value;
            constexpr int t = wtile(NT, I, kI);
            d4 x = acc[t];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double up = __shfl(x[r], lane + 2, 64);
                x[r] = colv ? x[r] : (fr == kc) ? fma(cc, up, x[r]) : 0.0;
            }
            acc[t] = x;
            wave_pin1<t>(acc[t]);
        });
        __builtin_amdgcn_sched_barrier(0);
    } else {
    if (conj && dbg != 2) {
        n0 = A.n0[w];
        WRows hs;
        hs.base = A.hf_panel; hs.ld = A.hf_ld;
        hs.ridx = (!LEAN && A.hf_row_idx) ? A.hf_row_idx + w * (long long)A.m : nullptr;
        hs.first = A.hf_start ? A.hf_start[w] : 0;
        hs.sub_row = nullptr;
        hs.count = A.hf_count ? A.hf_count[w] : A.m;
        hs.count0 = 0x7fffffff; hs.jump = 0;
        hs.off32 = (A.hf_off32 & 1) != 0;
        // ---- phase A: the shift row of the one-pass centred scatter (see posterior_fused_impl.h) = the window's first row
        const bool ones = kc < 15;        // a spare column k+1 carries ones; otherwise the sums are kept by vector adds (wave_gram)
        double shift[NT], w0v[NT], csum[NT];
        double usum = 0.0;
        {
            const long long row0 = hs.ridx ? (long long)hs.ridx[0] : hs.first;
            const double* p0 = hs.base + row0 * (long long)hs.ld;
#pragma unroll
            for (int i = 0; i < NT; ++i) {
                const int c = 16 * i + fr;
                const int cl = c < k ? c : k - 1;
                const double sv = p0[coff[i]];
                const double wv = A.w0[w * k + cl];
                shift[i] = sv;               // raw: zeroed beyond column k inside wave_gram (lazy_mask)
                w0v[i] = wv;
                csum[i] = 0.0;
            }
        }
        TP_MARK(1);
        // ---- phase B: Gram of the shifted intraday rows
        // the shift row is the window's FIRST row: shifted it is exactly zero and adds nothing to any sum, so the pass
        // starts at row 1 (77 intraday rows: 19 k-steps instead of 20); the means of phase C still divide by all rows
        const int hf_rows_all = hs.count;
        if (!hs.ridx) { hs.first += 1; hs.count -= 1; }
        else { hs.ridx += 1; hs.count -= 1; }
        if constexpr (!LEAN) wave_stage_rows(hs, lane, idx_rows_lds, idx_sub_lds);      // (WCfg::OFF_SUB)
        wave_gram<NT, 1, 0, true, LEAN>(hs, coff, k, lane, shift, w0v, ones, true, acc, idx_rows_lds, idx_sub_lds, csum, usum);
        hs.count = hf_rows_all;
        TP_MARK(2);
        // ---- phase C: rank-one term of the centring (one-pass form); q0, c, scaling (ref:333, 415-418).  ONE pass over
        // the tiles, a tile row at a time: vector instructions cannot read AGPRs, every tile visits the VGPR half on its
        // way - all 224 registers at once would spill, and a spill reload costs this lone wave a full memory round trip.
        const double invm = 1.0 / (double)hs.count;
        double tj[NT];
        double cz = corner();                                       // z'z = w0'C w0 (before the rank-one term)
        if (ones) {
            // column k+1 holds t_i = sum_r (y_r - s)_i for the asset columns and sum_r u_r in row k
            static_for<0, NT>([&](auto Ic) __attribute__((always_inline)) {
                constexpr int I = decltype(Ic)::value;
                constexpr int t = wtile(NT, I, kI);
                if (fr == kc + 1) {
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        lds[C::OFF_VEC + 16 * I + fq + 4 * r] = (I < kI || fq + 4 * r <= kc) ? acc[t][r] : 0.0;
                }
            });
        } else {
            // the same vector from the vector-add sums: the four row groups of a lane column meet by shuffles
#pragma unroll
            for (int i = 0; i < NT; ++i) {
                double sc_ = csum[i];
                sc_ += __shfl_xor(sc_, 16, 64);
                sc_ += __shfl_xor(sc_, 32, 64);
                if (fq == 0) lds[C::OFF_VEC + 16 * i + fr] = (16 * i + fr < k) ? sc_ : 0.0;
            }
            double su = usum;
            su += __shfl_xor(su, 16, 64);
            su += __shfl_xor(su, 32, 64);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            if (lane == 0) lds[C::OFF_VEC + k] = su;                // row k: sum_r u_r (over the zero the loop above put there)
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int J = 0; J < NT; ++J) tj[J] = lds[C::OFF_VEC + 16 * J + fr];          // column k: sum u; zero beyond
        {
            const double tk = lds[C::OFF_VEC + k];
            cz = fma(-(tk * invm), tk, cz);
        }
        const double mm = (double)hs.count;
        const double sc = n0 * (mm / (mm - 1.0));
        q0 = sc * cz;
        const double a = n0 + k + 2;
        cc = (2 * n0) / (a + sqrt(a * a + 4 * n0 * q0));
        // S0 = sc * C on the real columns, c * sc * C w0 in the border column, zero beyond
        const double fcol = colv ? sc : ((fr == kc) ? cc * sc : 0.0);
        static_for<0, NT>([&](auto Ic) __attribute__((always_inline)) {
            constexpr int I = decltype(Ic)::value;
            double ti[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) ti[r] = -(lds[C::OFF_VEC + 16 * I + fq + 4 * r] * invm);
            static_for<I, NT>([&](auto Jc) __attribute__((always_inline)) {
                constexpr int J = decltype(Jc)::value;
                constexpr int t = wtile(NT, I, J);
                d4 x = acc[t];
#pragma unroll
                for (int r = 0; r < 4; ++r) x[r] = fma(ti[r], tj[J], x[r]);
                if constexpr (J < kI) {
                    x *= sc;
                } else if constexpr (I < kI) {
                    x *= fcol;
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r) x[r] *= (fq + 4 * r < kc) ? fcol : 0.0;
                }
                acc[t] = x;
                wave_pin1<t>(acc[t]);
            });
            __builtin_amdgcn_sched_barrier(0);
        });
        __builtin_amdgcn_wave_barrier();
        if (dbg == 1) { dump_matrix(); return; }
    }
    TP_MARK(3);
    // ---- phase D: daily Gram (ref:180) + t in the border column (ref:222)
    {
        WRows ds;
        ds.base = A.panel; ds.ld = A.panel_ld;
        ds.ridx = (!LEAN && A.row_idx) ? A.row_idx + w * (long long)A.n_r : nullptr;
        ds.first = A.start ? A.start[w] : 0;
        ds.sub_row = A.rf_adj ? A.rf_adj + w * (long long)A.n_r : nullptr;
        ds.count = A.n_rows ? A.n_rows[w] : A.n_r;
        ds.count0 = 0x7fffffff; ds.jump = 0;
        ds.off32 = (A.panel_off32 & 1) != 0;
        double none[NT] = {};
        bool shared = false;
        const double* q = nullptr;
        if constexpr (LEAN) {
            // shared block-window sums (posterior_fused_impl.h, phase D): only the rows in front of the first whole
            // aligned 16-row block and behind the last one go through the MFMAs
            constexpr int BLK = 16;
            const long long b0 = (ds.first + BLK - 1) / BLK, b1 = (ds.first + ds.count) / BLK;
            const int Lw = (int)(b1 - b0);
            const int li = Lw == A.winsum_L[0] ? 0 : Lw == A.winsum_L[1] ? 1 : Lw == A.winsum_L[2] ? 2 : Lw == A.winsum_L[3] ? 3 : -1;
            shared = A.winsum != nullptr && Lw > 0 && li >= 0;
            if (shared) {
                ds.count0 = (int)(BLK * b0 - ds.first);
                ds.jump = (int)(BLK * b1 - ds.first) - ds.count0;
                ds.count = ds.count0 + (int)(ds.first + ds.count - BLK * b1);
                q = A.winsum + ((long long)li * A.prefix_nblk + b0) * ((long long)C::NTILES * 256);
            }
        }
        TP_MARK(32);
        // ONE table slot Q_L[b0]: [tile][2][64 lanes][2] doubles, two 16-byte reads per tile.  The reads run one group of
        // tiles ahead of the additions.
        typedef double d2 __attribute__((ext_vector_type(2)));
        constexpr int GRP = 7, NG = (C::NTILES + GRP - 1) / GRP;
        const d2* pq = (const d2*)q + lane;
        d2 qa[GRP][2], qb[GRP][2];
        auto qload = [&](d2 (&v2)[GRP][2], auto gc) __attribute__((always_inline)) {
            constexpr int g = decltype(gc)::value;
            static_for<0, GRP>([&](auto ec) __attribute__((always_inline)) {
                constexpr int e = decltype(ec)::value;
                constexpr int t = g * GRP + e;
                if constexpr (t < C::NTILES) {
                    v2[e][0] = pq[(long long)t * 128];
                    v2[e][1] = pq[(long long)t * 128 + 64];
                }
            });
        };
        auto qadd = [&](d2 (&v2)[GRP][2], auto gc) __attribute__((always_inline)) {
            constexpr int g = decltype(gc)::value;
            static_for<0, GRP>([&](auto ec) __attribute__((always_inline)) {
                constexpr int e = decltype(ec)::value;
                constexpr int t = g * GRP + e;
                if constexpr (t < C::NTILES) {
                    d4 x = acc[t];
                    x[0] += v2[e][0][0]; x[1] += v2[e][0][1];
                    x[2] += v2[e][1][0]; x[3] += v2[e][1][1];
                    acc[t] = x;
                    wave_pin1<t>(acc[t]);
                }
            });
        };
        // (every load of the intraday pass has completed: its staging region is free for the daily pass)
        if constexpr (!LEAN) wave_stage_rows(ds, lane, idx_rows_lds, idx_sub_lds);
        double nosum = 0.0;
        wave_gram<NT, 1, 0, false, LEAN>(ds, coff, k, lane, none, none, false, false, acc, idx_rows_lds, idx_sub_lds, none, nosum);
        TP_MARK(33);
        if (LEAN && shared) {
            // (issuing the first group in front of the edge rows' loop was measured and dropped: the loop's counted
            // vmcnt waits then also wait for the table reads - 0.648 vs 0.593 ms at configs[1])
            qload(qa, ic<0>{});
            static_for<0, NG>([&](auto gc) __attribute__((always_inline)) {
                constexpr int g = decltype(gc)::value;
                if constexpr (g + 1 < NG) {
                    if constexpr (g % 2 == 0) qload(qb, ic<g + 1>{}); else qload(qa, ic<g + 1>{});
                }
                __builtin_amdgcn_sched_barrier(0);
                if constexpr (g % 2 == 0) qadd(qa, gc); else qadd(qb, gc);
                __builtin_amdgcn_sched_barrier(0);
            });
        }
    }
    }   // !PRE
    TP_MARK(34);
    // rows >= k of the bordered matrix are never pivots: clear them (they hold 1'X, n_r, ...)
    static_for<0, NT>([&](auto Ic) __attribute__((always_inline)) {
        constexpr int I = decltype(Ic)::value;
        constexpr int t = wtile(NT, I, kI);
        if constexpr (I == kI) {
            d4 x = acc[t];
#pragma unroll
            for (int r = 0; r < 4; ++r) x[r] = (fq + 4 * r >= kc) ? 0.0 : x[r];
            acc[t] = x;
            wave_pin1<t>(acc[t]);
        }
    });
    __builtin_amdgcn_sched_barrier(0);
    if (dbg == 2) { dump_matrix(); return; }

    if (!conj) {
        // ---- phase E: J = T - t t'/N (ref:600-601); t stays in the border column (ref:606 rhs)
        static_for<0, NT>([&](auto Ic) __attribute__((always_inline)) {
            constexpr int I = decltype(Ic)::value;
            constexpr int t = wtile(NT, I, kI);
            if (fr == kc) {
#pragma unroll
                for (int r = 0; r < 4; ++r) lds[C::OFF_VEC + 16 * I + fq + 4 * r] = acc[t][r];
            }
        });
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const double invN = !FULL ? 1.0 / (double)A.N : A.center_rows == 2 ? 0.0
                          : 1.0 / (double)(A.center_rows ? (A.n_rows ? A.n_rows[w] : A.n_r) : A.N);
        const double sh_d = (FULL && A.shift) ? A.shift[2 * w] : 0.0;
        const double sh_e = (FULL && A.shift) ? A.shift[2 * w + 1] : 0.0;
        double tj[NT];
#pragma unroll
        for (int J = 0; J < NT; ++J) tj[J] = lds[C::OFF_VEC + 16 * J + fr];
        static_for<0, NT>([&](auto Ic) __attribute__((always_inline)) {
            constexpr int I = decltype(Ic)::value;
            double ti[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) ti[r] = lds[C::OFF_VEC + 16 * I + fq + 4 * r];
            static_for<I, NT>([&](auto Jc) __attribute__((always_inline)) {
                constexpr int J = decltype(Jc)::value;
                constexpr int t = wtile(NT, I, J);
                d4 x = acc[t];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const bool on = (J < kI || colv) && (I < kI || fq + 4 * r < kc);
                    const double add = sh_e + ((I == J && fq + 4 * r == fr) ? sh_d : 0.0);
                    x[r] += on ? add - invN * (ti[r] * tj[J]) : 0.0;
                }
                acc[t] = x;
                wave_pin1<t>(acc[t]);
            });
            __builtin_amdgcn_sched_barrier(0);
        });
        __builtin_amdgcn_wave_barrier();
    }
    if (FULL && A.rhs != nullptr) {
        static_for<0, NT>([&](auto Ic) __attribute__((always_inline)) {
            constexpr int I = decltype(Ic)::value;
            constexpr int t = wtile(NT, I, kI);
            if (fr == kc) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int gi = 16 * I + fq + 4 * r;
                    const int gl = gi < k ? gi : k - 1;
                    const double x = A.rhs[w * k + gl];
                    acc[t][r] = (gi < k) ? x : 0.0;
                }
            }
            wave_pin1<t>(acc[t]);
        });
    }
    if (FULL && A.out_rhs != nullptr) {
        static_for<0, NT>([&](auto Ic) __attribute__((always_inline)) {
            constexpr int I = decltype(Ic)::value;
            constexpr int t = wtile(NT, I, kI);
            if (fr == kc) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int gi = 16 * I + fq + 4 * r;
                    if (gi < k) A.out_rhs[w * k + gi] = acc[t][r];
                }
            }
        });
    }
    if (dbg == 3) dump_matrix();
    if constexpr (POST) {
        // the matrix is complete (phase E applied): keep it before phase F factorises it in place
        double* P = tp_post_window(A, w);
        if (P != nullptr) {
            static_for<0, NT>([&](auto Ic) __attribute__((always_inline)) {
                constexpr int I = decltype(Ic)::value;
                static_for<I, NT>([&](auto Jc) __attribute__((always_inline)) {
                    constexpr int J = decltype(Jc)::value;
                    wave_post_tile<I, J>(P, k, fr, fq, acc[wtile(NT, I, J)]);
                });
            });
        }
    }

    TP_MARK(4);
    // ---- phase F: blocked upper Cholesky S1 = R'R with the border column riding along (y = R^-T b)
    double badacc = 0.0;
    static_for<0, NT>([&](auto jc) __attribute__((always_inline)) {
        constexpr int j = decltype(jc)::value;
        if (j < NTB) {
            const int npiv = (k - 16 * j < 16) ? (k - 16 * j) : 16;
            constexpr int tjj = wtile(NT, j, j);
            // (1) diagonal tile -> LDS (row-major) -> one column per lane; lanes 16-31 take the identity's columns
#pragma unroll
            for (int r = 0; r < 4; ++r) lds[C::OFF_DG + (fq + 4 * r) * 16 + fr] = acc[tjj][r];
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            const int c16 = lane & 15;
            double a[16];
            const double* src = (lane < 16) ? (lds + C::OFF_DG) : (lds + C::OFF_IDT);
#pragma unroll
            for (int i = 0; i < 16; ++i) a[i] = src[i * 16 + c16];
            // (2) 16 pivots, rsqrt (v_rsq_f64 + one cubic step) with look-ahead.  Block rows in front of the last one have
            // 16 live pivots at compile time (no selects).  A non-positive or NaN pivot makes its 1/sqrt an infinity or a
            // NaN: 0 * rinv is accumulated per pivot (ONE instruction) and looked at once.
            // The scaled pivot row IS the multipliers of the rows below it: lane i holds row i's.
            //  * The next diagonal element never leaves its lane: lane p+1 holds t = a[p] and a[p+1], and fma(-t, t, a[p+1])
            //    there is the very fma the row update performs, so the next pivot's 1/sqrt is computed lane-locally and ONE
            //    v_readlane pair of the finished value is left on the serial path (before: multiplier, update, diagonal, rsqrt).
            //  * Rows p+1 and p+2 - what the next pivot and its own look-ahead wait for - take their multipliers by
            //    v_readlane; every other row reads its multiplier from LDS: lanes 0..15 write the scaled pivot row to one of
            //    two 16-double rows (by pivot parity: a write never meets the previous pivot's reads) at the front of the
            //    OFF_DG region - free since a[] was loaded - and all lanes read it back at lane-uniform addresses (a
            //    broadcast), two multipliers per ds_read_b128.  Lanes 16..63 write behind the two rows, so no exec mask is
            //    switched.  The fma gets the same multiplier in the same operand position: every result keeps its bits.
            constexpr bool ALL16 = j < kI;
            constexpr int RL = 2;                                     // rows per pivot that keep the v_readlane form
            typedef double d2 __attribute__((ext_vector_type(2)));
            double* const mrows = lds + C::OFF_DG;
            const int mw = (lane < 16) ? lane : 32 + lane;
            double d0 = readlane_d(a[0], 0);
            double rinv = rsqrt_cubic(d0);
#pragma unroll
            for (int p = 0; p < 16; ++p) {
                if (ALL16 || p < npiv) {
                    a[p] *= rinv;
                    badacc = fma(0.0, rinv, badacc);
                    const int i0 = p + 1 + RL;                       // first row whose multiplier comes from LDS
                    double* const mrow = mrows + 16 * (p & 1);
                    if (i0 < 16) {
                        mrow[mw] = a[p];
                        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                        __builtin_amdgcn_wave_barrier();
                    }
                    double mm[16];
#pragma unroll
                    for (int i = i0; i < 16; ++i) {
                        if ((i & 1) == 0) {
                            const d2 v = *(const d2*)(mrow + i);
                            mm[i] = v[0];
                            mm[i + 1] = v[1];
                        } else if (i == i0) {
                            mm[i] = mrow[i];
                        }
                    }
                    double rinv_next = 1.0;
                    if (p + 1 < 16) {
                        double dn = fma(-a[p], a[p], a[p + 1]);      // lane p+1: the next diagonal element
                        if (!ALL16) dn = (p + 1 < npiv) ? dn : 1.0;
                        rinv_next = readlane_d(rsqrt_cubic(dn), p + 1);
                    }
#pragma unroll
                    for (int i = p + 1; i < i0 && i < 16; ++i) {
                        const double sI = readlane_d(a[p], i);
                        a[i] = fma(-sI, a[p], a[i]);
                    }
#pragma unroll
                    for (int i = i0; i < 16; ++i) a[i] = fma(-mm[i], a[p], a[i]);
                    rinv = rinv_next;
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            // M_j = R_jj^-T (lower triangular), rows past the last pivot zeroed
            if (lane >= 16 && lane < 32) {
#pragma unroll
                for (int i = 0; i < 16; ++i) lds[C::OFF_M + (j * 16 + i) * C::MLD + c16] = (i < npiv) ? a[i] : 0.0;
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            // (3) block row j: R_jJ = M A_jJ (A operand: M, B operand: the tile's own registers)
            double mop[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) mop[r] = lds[C::OFF_M + (j * 16 + fr) * C::MLD + 4 * r + fq];    // M[fr][4r + fq]
            static_for<j, NT>([&](auto Jc) __attribute__((always_inline)) {
                constexpr int J = decltype(Jc)::value;
                if constexpr (J > j || j == kI) {        // R_jj itself is never used again (the solves use M_j)
                    constexpr int t = wtile(NT, j, J);
                    d4 rj = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
                    for (int r = 0; r < 4; ++r) rj = __builtin_amdgcn_mfma_f64_16x16x4f64(mop[r], acc[t][r], rj, 0, 0, 0);
                    acc[t] = rj;
                }
            });
            // (4) trailing update A_IJ -= R_jI' R_jJ, operands straight from the block row's registers
            static_for<j + 1, NT>([&](auto Ic) __attribute__((always_inline)) {
                constexpr int I = decltype(Ic)::value;
                static_for<I, NT>([&](auto Jc) __attribute__((always_inline)) {
                    constexpr int J = decltype(Jc)::value;
                    constexpr int t = wtile(NT, I, J), tI = wtile(NT, j, I), tJ = wtile(NT, j, J);
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(acc[tI][r], acc[tJ][r], acc[t], 0, 0, 1);
                });
            });
        }
    });

    TP_MARK(5);
    // ---- phase G: y, q1 = y'y (ref:574), back substitution R w = y along block rows
    double q1 = 0.0;
    double wcol[NT];          // wcol[J] = w[16 J + fr] in every lane group
#pragma unroll
    for (int J = 0; J < NT; ++J) wcol[J] = 0.0;
    {
        double q1p = 0.0;
        static_for<0, NT>([&](auto Ic) __attribute__((always_inline)) {
            constexpr int I = decltype(Ic)::value;
            constexpr int t = wtile(NT, I, kI);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double y = (fr == kc && (I < kI || fq + 4 * r < kc)) ? acc[t][r] : 0.0;
                q1p = fma(y, y, q1p);
            }
        });
        q1 = wave_sum64(q1p);
    }
    static_for<0, NT>([&](auto ic) __attribute__((always_inline)) {
        constexpr int Ib = NT - 1 - decltype(ic)::value;
        if (Ib < NTB) {
            constexpr int tb = wtile(NT, Ib, kI);
            // z_r (rows 4r + fq of block Ib) = y - sum_{J > Ib} R_{Ib,J} w_J: lane-local products, ONE reduction per register
            double z[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                double u = 0.0;
                static_for<Ib + 1, NT>([&](auto Jc) __attribute__((always_inline)) {
                    constexpr int J = decltype(Jc)::value;
                    constexpr int t = wtile(NT, Ib, J);
                    if (J < NTB) u = fma(acc[t][r], wcol[J], u);
                });
                // the border column's y sits in lane fr == kc of its 16-lane row group: it joins the same reduction
                const double y = (fr == kc && (Ib < kI || fq + 4 * r < kc)) ? acc[tb][r] : 0.0;
                z[r] = rowgroup_sum16(y - u);
            }
            // w_Ib = M' z by MFMA: A[i][kk] = z[4r + kk] (any i), B[kk][n] = M[4r + kk][n]  =>  every row of the result is w'
            d4 wt = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double mrow = lds[C::OFF_M + (Ib * 16 + 4 * r + fq) * C::MLD + fr];
                wt = __builtin_amdgcn_mfma_f64_16x16x4f64(z[r], mrow, wt, 0, 0, 0);
            }
            wcol[Ib] = wt[0];
            __builtin_amdgcn_sched_barrier(0);
        }
    });

    TP_MARK(6);
    // ---- phase H: weights, status, aux (ref:572-575, 836 / 849)
    {
        const double n1 = n0 + (double)A.N;
        const double denom = n1 - q1;
        bool nonfinite = false;
        static_for<0, NT>([&](auto Ic) __attribute__((always_inline)) {
            constexpr int I = decltype(Ic)::value;
            const int gi = 16 * I + fr;
            double out;
            if (conj) out = 1.0 / A.gamma * ((n1 + k + 2) * wcol[I] / denom);
            else out = 1.0 / A.gamma * wcol[I];
            if (fq == (I & 3) && gi < k) {
                A.weights[w * k + gi] = out;
                if (!isfinite(out)) nonfinite = true;
            }
        });
        const bool anybad = __any(nonfinite ? 1 : 0) != 0;
        const bool notpd = __any((badacc != badacc) ? 1 : 0) != 0;
        if (lane == 0) {
            int st = TP_KSTATUS_OK;
            if (notpd) st = TP_KSTATUS_NOT_PD;
            else if (anybad) st = TP_KSTATUS_NONFINITE;
            else if (conj && !(denom > 0.0)) st = TP_KSTATUS_BAD_DENOM;
            A.status[w] = st;
            if (A.aux) {
                double* ax = A.aux + w * 8;
                ax[0] = n0; ax[1] = conj ? n1 : 0.0; ax[2] = cc; ax[3] = q0; ax[4] = q1;
                ax[5] = conj ? denom : 0.0; ax[6] = 0.0; ax[7] = 0.0;
            }
        }
    }
    TP_MARK(7);
}

// Windows (= waves) per SIMD the register allocator is asked to keep: the accumulators take 8 registers per tile, the
// row pipeline about 100; two or more waves per SIMD also double the vector issue rate (one wave alone issues an fp64
// vector instruction every ~9 cycles, two get one every ~4.75: tools/coexec_probe.hip).
constexpr int wave_occupancy(int nt) { return nt <= 3 ? 4 : nt <= 5 ? 2 : 1; }

template <int NT, bool LEAN, int MODE>
__global__ void __launch_bounds__(64, wave_occupancy(NT)) posterior_wave_kernel(const tp_kargs_t A) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    wave_window_body<NT, LEAN, MODE>(A, lds);
}

// the PRE form (wave_window_body): contiguous layout, MODE 0 / 3
template <int NT, int MODE>
__global__ void __launch_bounds__(64, wave_occupancy(NT)) posterior_wave_kernel_pre(const tp_kargs_t A) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    wave_window_body<NT, true, MODE, true>(A, lds);
}
// Does a batch run the PRE form?  Plain conjugate on the contiguous layout (the caller's MODE / LEAN), shared tables with
// their all-zero slot (the host leaves winsum_zero null where a prior strength or an intraday row count rules the scaled
// rows out: plan_shared_gram), columns k+1 and k+2 inside tile column kI, and the option (tp_kopts_t::wave_preload).
// Where the automatic choice takes it: measured per tile count (alternating runs against the parent build, 10,000 windows,
// profiles/r19_wave_preload_bench.txt).  It pays where the form with the two passes over the tiles spills - 5 tiles per side
// (k = 77: -15 %), 7 (k = 100: -3 %), 8 and 9 (k = 120, 140: -21 %, -23 %) - and is +- 0 where neither form spills (k = 55,
// 90: 4 and 6 tiles); 1 to 3 tiles per side were not measured.  wave_preload = 1 runs it wherever the batch is eligible.
// With the centring row inside the edge rows' last k-step (profiles/r26_centring_row_bench.txt) wave_preload = 1 gains 1.7 %
// and 1.9 % at 4 and 6 tiles per side as well; the automatic choice there is left as it was until the suite has run on it.
constexpr bool wave_preload_pays(int nt) { return nt == 5 || nt >= 7; }
template <int NT>
inline bool wave_preload_eligible(const tp_kargs_t& a) {
    const bool wanted = a.opts.wave_preload == 1 || (a.opts.wave_preload < 0 && wave_preload_pays(NT));
    return wanted && a.winsum != nullptr && a.winsum_zero != nullptr && a.strategy == 0 && a.k - 16 * (NT - 1) <= 13;
}

// LDS bytes of a launch: the fixed image, plus the staging region of the general layout (sized by the batch's passes)
template <int NT, bool LEAN>
inline int wave_lds_bytes(const tp_kargs_t& a) {
    return WCfg<NT, LEAN>::LDS_BYTES + (LEAN ? 0 : wave_idx_bytes(a.n_r, a.m, a.strategy == 0));
}

// Instantiations with the posterior store that are not built: in the general-layout conjugate kernel of 8 tiles per side the
// store's extra live values make the register allocator move an accumulator tile between the register files INSIDE the row
// loop (a read of an MFMA result too soon after its issue: tools/check_mfma_hazards.py rejects it).  Such a batch keeps its
// matrices on the multi-wave kernel (hipErrorNotSupported: launch_one falls back).
constexpr bool wave_post_built(int nt, bool lean, int mode) { return !(mode == 3 && nt == 8 && !lean); }

template <int NT, bool LEAN, int MODE>
hipError_t wave_launch_mode(const tp_kargs_t& a, int grid8, hipStream_t stream) {
    if constexpr (!wave_post_built(NT, LEAN, MODE)) {
        return hipErrorNotSupported;
    } else {
        const int lds_bytes = wave_lds_bytes<NT, LEAN>(a);
        if (lds_bytes > WAVE_LDS_LIMIT) return hipErrorNotSupported;     // nothing launched: launch_one falls back to the multi-wave kernel
        static std::atomic<unsigned long long> attr_done{0};      // one bit per device (tp_allow_dynamic_lds)
        { hipError_t e = tp_allow_dynamic_lds(attr_done, posterior_wave_kernel<NT, LEAN, MODE>, WAVE_LDS_LIMIT); if (e != hipSuccess) return e; }
        hipLaunchKernelGGL((posterior_wave_kernel<NT, LEAN, MODE>), dim3(grid8), dim3(64), lds_bytes, stream, a);
        return hipGetLastError();
    }
}

template <int NT, int MODE>
hipError_t wave_launch_pre(const tp_kargs_t& a, int grid8, hipStream_t stream) {
    const int lds_bytes = wave_lds_bytes<NT, true>(a);
    static std::atomic<unsigned long long> attr_done{0};      // one bit per device (tp_allow_dynamic_lds)
    { hipError_t e = tp_allow_dynamic_lds(attr_done, posterior_wave_kernel_pre<NT, MODE>, WAVE_LDS_LIMIT); if (e != hipSuccess) return e; }
    hipLaunchKernelGGL((posterior_wave_kernel_pre<NT, MODE>), dim3(grid8), dim3(64), lds_bytes, stream, a);
    return hipGetLastError();
}

template <int NT, bool LEAN>
hipError_t wave_launch_variant(const tp_kargs_t& a, int grid, hipStream_t stream, tp_launch_info_t* info) {
    if (info) { info->grid = grid; info->block = 64; info->lds_bytes = wave_lds_bytes<NT, LEAN>(a); info->ntile = NT; }
    const int grid8 = 8 * ((grid + 7) / 8);
    const int mode = wave_mode(a);
    if constexpr (LEAN) {
        if (mode == 0 && wave_preload_eligible<NT>(a))
            return a.out_post != nullptr ? wave_launch_pre<NT, 3>(a, grid8, stream) : wave_launch_pre<NT, 0>(a, grid8, stream);
    }
    switch (mode == 2 ? 2 : tp_post_mode(a, mode)) {
        case 0: return wave_launch_mode<NT, LEAN, 0>(a, grid8, stream);
        case 1: return wave_launch_mode<NT, LEAN, 1>(a, grid8, stream);
        case 3: return wave_launch_mode<NT, LEAN, 3>(a, grid8, stream);
        case 4: return wave_launch_mode<NT, LEAN, 4>(a, grid8, stream);
        default: return hipErrorNotSupported;        // launch_one keeps such batches on the multi-wave kernel
    }
}

}  // namespace
