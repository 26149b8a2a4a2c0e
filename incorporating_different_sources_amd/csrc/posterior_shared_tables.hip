// posterior_shared_tables.hip - the block-window tables Q_L of the register-tile path straight from the daily panel, in
// one kernel.  It replaces the pair block_gram_kernel + tp_window_sums_kernel: the block Grams G
// are never written to memory and never read back, and there is no kernel boundary between the two.
//
// A wave owns ONE 16 x 16 tile (I, J) of the slot, for one group of R = min(L, 16) consecutive positions g .. g + R - 1 of
// one table L (the groups of tp_window_sums_kernel: cut at multiples of R, absolute positions).  It forms the tile of
// every block Gram it needs itself, with the operands and the k-step order of block_gram_kernel (gram_phase_lean<C,
// false, -1>): lane (fq, fr) holds row 4 s + fq, columns 16 I + fr and 16 J + fr of the block - the panel value below
// column k (padding lanes load column k - 1 and drop it), 1.0 in column k, 0.0 beyond - the accumulator starts at zero
// and the 4 (32-row blocks: 8) k-steps run in ascending order.  Then the additions of tp_window_sums_kernel, element by
// element and in its order, the additions to a zero run / M / P included:
//     S[i] = G[g+i] + (.. + (G[g+R-1] + 0))       backwards over the group's own blocks
//     M    = (0 + G[g+R]) + .. + G[g+L-1]          forwards, empty for L <= 16
//     out[g] = S[0] + M;   P = (0 + G[g+L]) + .. ;   out[g+i] = (S[i] + M) + P
// so every table element has the bits the pair gives it, and - additions only - a NaN or huge row spoils exactly the
// windows that contain it.  (M is formed FIRST here, while no suffix sum occupies registers: the three sums are
// independent of each other until out[] adds them, so their order in time changes no bit.)  The blocks a wave needs are
// one descending run g+R-1 .. g and one ascending run g+R .. g+L+R-2: 2 R - 1 block tiles for R positions when L <= 16.
// Their loads depend on nothing that is computed: a ring of ST_PF entries of 4 k-steps' operands is kept in flight
// ahead of the MFMAs.  No LDS.  The 4 waves of a workgroup take 4 consecutive tiles of the row-major upper triangle, which
// mostly share a tile row: their A operands are the same cache lines.
//
// The kernel is templated on the k-steps per block alone: the tile count and the tile coordinates are wave-uniform
// run-time values (one accumulator tile per wave: nothing is indexed by them), so one instantiation serves NT = 1..12
// and one NT = 13..15.  Inside, the body is instantiated per group length R: the suffix sums S[0..R-1] are 8 R registers
// that must be indexed by constants.
#include "posterior_kernels.h"
#include <type_traits>

namespace {

typedef double st_d2 __attribute__((ext_vector_type(2)));
typedef double st_d4 __attribute__((ext_vector_type(4)));

// operands of 4 k-steps (16 rows): what one ring entry holds.  A 16-row block is one of them, a 32-row block two.
struct QuadOps { double a[4], b[4]; };

struct TableArgs {
    const double* panel;
    st_d2* Q;
    long long slot_pairs;   // 16-byte pairs per slot
    int ld, k, nt, nblk;
    int L[TP_WINSUM_MAX_L];
    int n_L;
    int nquads, gpx;        // workgroups (4 tiles each) per slot; groups per XCD
};

// ring entries in flight ahead of the MFMAs (16 registers each); the scheduler is held to this depth (sched_barrier):
// left alone it hoists more loads than the registers beside the suffix sums can take, and spills
constexpr int ST_PF = 4;

// RR: group length; MID: L > 16 (then RR = 16 and the middle sum M is not empty)
template <int KS, int RR, bool MID>
__device__ __forceinline__ void tables_body(const TableArgs& A, int L, int g, int npos, unsigned oA, unsigned oB, bool vA, bool vB,
                                            double fA, double fB, char* out, unsigned ol) {
    constexpr int PF = ST_PF, QB = KS / 4;                     // QB: ring entries per block
    static_assert(KS == 4 || KS == 8, "16- or 32-row blocks");
    const int last = A.nblk - 1;
    const long long ld8 = 8ll * A.ld, sp16 = 16 * A.slot_pairs;
    // entry h of block b.  Addresses are a wave-uniform 64-bit base (scalar registers: block, entry and k-step) plus the
    // lane's 32-bit byte offset of (row fq, column): no vector instruction and no vector register goes into an address
    auto load = [&](QuadOps& o, int b, int h) __attribute__((always_inline)) {
        const int bc = __builtin_amdgcn_readfirstlane(b < last ? b : last);      // never past the panel's whole blocks
        const char* ub = (const char*)A.panel + ((long long)bc * (4 * KS) + 16 * h) * ld8;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const char* us = ub + (4 * s) * ld8;
            o.a[s] = *(const double*)(us + (size_t)oA);
            o.b[s] = *(const double*)(us + (size_t)oB);
        }
    };
    auto mfma4 = [&](const QuadOps& o, st_d4 acc) __attribute__((always_inline)) {
#pragma unroll
        for (int s = 0; s < 4; ++s)
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(vA ? o.a[s] : fA, vB ? o.b[s] : fB, acc, 0, 0, 0);
        return acc;
    };
    auto put = [&](int p, const st_d4& v) __attribute__((always_inline)) {
        char* uq = out + (long long)__builtin_amdgcn_readfirstlane(p) * sp16;   // uniform; the lane adds its 16 bytes
        *(st_d2*)(uq + (size_t)ol) = st_d2{v[0], v[1]};
        *(st_d2*)(uq + (size_t)ol + 1024) = st_d2{v[2], v[3]};
    };
    const st_d4 zero = st_d4{0.0, 0.0, 0.0, 0.0};
    QuadOps ring[PF];
    st_d4 S[RR];
    st_d4 M = zero, P = zero, run = zero, acc = zero;

    // A static stream of T blocks (block number blk(n)), PF ring entries ahead; done(n, G) takes the n-th block's tile Gram
    auto stream = [&](auto Tc, auto blk, auto done) __attribute__((always_inline)) {
        constexpr int T = decltype(Tc)::value;
#pragma unroll
        for (int m = 0; m < PF; ++m)
            if (m < T * QB) load(ring[m], blk(m / QB), m % QB);
#pragma unroll
        for (int m = 0; m < T * QB; ++m) {
            if (m % QB == 0) acc = zero;
            acc = mfma4(ring[m % PF], acc);
            if (m + PF < T * QB) load(ring[m % PF], blk((m + PF) / QB), (m + PF) % QB);
            __builtin_amdgcn_sched_barrier(0);
            if (m % QB == QB - 1) done(m / QB, acc);
        }
    };
    auto suffix = [&](int n, const st_d4& G) __attribute__((always_inline)) {     // n-th block from the group's end
        run = run + G;
        S[RR - 1 - n] = run;
    };
    auto prefix = [&](int i, const st_d4& G) __attribute__((always_inline)) {     // position g + i, i >= 1
        if (g + i < npos) {
            P = P + G;
            put(g + i, (S[i] + M) + P);
        }
    };

    if constexpr (MID) {
        static_assert(!MID || RR == TP_WINSUM_RUN, "a middle sum exists behind whole groups only");
        // The middle first, while no suffix sum is live: M does not depend on them, and out[g] needs both anyway.  Rounds
        // of MR ring entries of their own, loaded together.
        constexpr int MR = 8, PB = MR / QB;                    // entries, blocks per round
        QuadOps mid[MR];
#pragma nounroll
        for (int b = g + RR; b < g + L; b += PB) {
#pragma unroll
            for (int m = 0; m < MR; ++m) load(mid[m], b + m / QB, m % QB);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int j = 0; j < PB; ++j) {
                acc = zero;
#pragma unroll
                for (int h = 0; h < QB; ++h) acc = mfma4(mid[j * QB + h], acc);
                if (b + j < g + L) M = M + acc;
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    // one stream: blocks g+RR-1 .. g (suffix sums), then g+L .. g+L+RR-2 (prefixes)
    stream(std::integral_constant<int, 2 * RR - 1>{},
           [&](int n) __attribute__((always_inline)) { return n < RR ? g + RR - 1 - n : g + L + n - RR; },
           [&](int n, const st_d4& G) __attribute__((always_inline)) {
               if (n < RR) {
                   suffix(n, G);
                   if (n == RR - 1) put(g, S[0] + M);
               } else {
                   prefix(n - RR + 1, G);
               }
           });
}

template <int KS>
__global__ void __launch_bounds__(256, 2) tp_shared_tables_kernel(const TableArgs A) {
    const int wv = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    // Workgroups go round the 8 XCDs by their number: an XCD takes a contiguous range of groups, for every tile and every
    // table, so that its L2 holds one eighth of the panel's blocks (plus L - 1 behind each range) and not all of them
    const int id = blockIdx.x, xcd = id & 7;
    int rest = id >> 3;
    const int quad = rest % A.nquads; rest /= A.nquads;
    const int gl = rest % A.gpx, li = rest / A.gpx;
    const int t = quad * 4 + wv;                               // tile of this wave, row-major over the upper triangle
    if (t >= A.nt * (A.nt + 1) / 2 || li >= A.n_L) return;
    int I = 0, rem = t;
    while (rem >= A.nt - I) { rem -= A.nt - I; ++I; }
    const int J = I + rem;
    const int L = li == 0 ? A.L[0] : li == 1 ? A.L[1] : li == 2 ? A.L[2] : A.L[3];
    if (L < 1) return;
    const int npos = A.nblk - L + 1;                           // positions b0 with b0 + L <= nblk
    const int Rr = L < TP_WINSUM_RUN ? L : TP_WINSUM_RUN;      // group length
    const long long g64 = (long long)(xcd * A.gpx + gl) * Rr;  // first position of the group (absolute: table position 0 is block 0)
    if (g64 >= npos) return;
    const int g = (int)g64;
    const int fr = lane & 15, fq = lane >> 4;
    const int cA = 16 * I + fr, cB = 16 * J + fr, k = A.k;
    const bool vA = cA < k, vB = cB < k;
    const double fA = cA == k ? 1.0 : 0.0, fB = cB == k ? 1.0 : 0.0;   // the ones column, zeros beyond it
    const unsigned oA = 8u * (unsigned)(fq * A.ld + (vA ? cA : k - 1));   // 4 ld doubles: far below 2^32 bytes (plan_shared_gram)
    const unsigned oB = 8u * (unsigned)(fq * A.ld + (vB ? cB : k - 1));
    char* out = (char*)(A.Q + (long long)li * A.nblk * A.slot_pairs + (long long)t * 128);
    const unsigned ol = 16u * (unsigned)lane;
    if (L > TP_WINSUM_RUN) { tables_body<KS, TP_WINSUM_RUN, true>(A, L, g, npos, oA, oB, vA, vB, fA, fB, out, ol); return; }
    switch (Rr) {
#define TP_ST_CASE(R) case R: tables_body<KS, R, false>(A, L, g, npos, oA, oB, vA, vB, fA, fB, out, ol); break;
        TP_ST_CASE(1) TP_ST_CASE(2) TP_ST_CASE(3) TP_ST_CASE(4) TP_ST_CASE(5) TP_ST_CASE(6) TP_ST_CASE(7) TP_ST_CASE(8)
        TP_ST_CASE(9) TP_ST_CASE(10) TP_ST_CASE(11) TP_ST_CASE(12) TP_ST_CASE(13) TP_ST_CASE(14) TP_ST_CASE(15) TP_ST_CASE(16)
#undef TP_ST_CASE
        default: break;
    }
}

}  // namespace

// The automatic choice, per tile count: the one kernel wherever it measured faster than the pair (DESIGN.md section 4a,
// profiles/r23_shared_tables_bench.txt: every tile count 1 .. 12, by 1.3 % (k = 55) to 9 % (k = 10) of the step).  With
// 32-row blocks (13 .. 15 tiles per side) it measured -0.2 % at 13 and 15, no more than twice the parent's spread, and
// nothing at 14: those keep the pair; shared_tables = 1 runs the one kernel there too.
bool tp_shared_tables_pays(int nt) { return nt <= 12; }

hipError_t tp_shared_tables_launch(const double* panel, int ld, int k, double* Q, int nblk, const int* L, int n_L,
                                   hipStream_t stream) {
    if (n_L < 1 || nblk < 1) return hipSuccess;
    if (n_L > TP_WINSUM_MAX_L || k < 1 || ld < k) return hipErrorInvalidValue;
    TableArgs A;
    A.panel = panel; A.Q = (st_d2*)Q; A.ld = ld; A.k = k; A.nblk = nblk; A.n_L = n_L;
    A.nt = (k + 1 + 15) / 16;
    const int ntiles = A.nt * (A.nt + 1) / 2;
    A.slot_pairs = (long long)ntiles * 128;
    int groups = 0;                                            // the largest group count among the tables
    for (int i = 0; i < TP_WINSUM_MAX_L; ++i) {
        A.L[i] = i < n_L ? L[i] : 0;
        const int Rr = A.L[i] < TP_WINSUM_RUN ? A.L[i] : TP_WINSUM_RUN;
        const int npos = nblk - A.L[i] + 1;
        if (Rr >= 1 && npos >= 1 && (npos + Rr - 1) / Rr > groups) groups = (npos + Rr - 1) / Rr;
    }
    if (groups < 1) return hipSuccess;
    A.nquads = (ntiles + 3) / 4;
    A.gpx = (groups + 7) / 8;
    const long long wgs = 8ll * A.nquads * A.gpx * n_L;
    if (wgs > 0x7fffffffLL) return hipErrorInvalidValue;
    const dim3 grid((unsigned)wgs);
    if (TP_PREFIX_BLOCK_ROWS(A.nt) == 16) hipLaunchKernelGGL(tp_shared_tables_kernel<4>, grid, dim3(256), 0, stream, A);
    else hipLaunchKernelGGL(tp_shared_tables_kernel<8>, grid, dim3(256), 0, stream, A);
    return hipGetLastError();
}
