// posterior_kernels.h - internal interface between the host layer (tangency_api.cpp, tangency_sweep.cpp) and the HIP kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#define TP_KSTATUS_OK 0
#define TP_KSTATUS_NOT_PD 1
#define TP_KSTATUS_NONFINITE 2
#define TP_KSTATUS_BAD_DENOM 3

// Kernel-selection switches of a handle (A/B measurements and tests).  -1 = automatic.  Read from the environment once,
// in tp_create (TP_WAVE_KERNEL, TP_TILED_WAVE, TP_TILED_FUSE), changed through tp_set_option; the launchers read
// them from the batch's arguments, never from the environment.
struct tp_kopts_t {
    int wave_kernel = -1;   // register-tile path: 0 = multi-wave kernel, 1 = one-wave kernel (k <= 143), 2 = two-wave kernel
    int tiled_wave = -1;    // large-k path: 0 = the 4-wave Gram / diagonal-block kernels, 1 = the one-wave kernels (-1, 0, 1 only)
    int tiled_fuse = -1;    // large-k path: 0 / 1 = three-kernel / fused left-looking update + solve
    int wave_preload = -1;  // one-wave kernel, accumulators started from the table slot: 0 = never, 1 = wherever the batch is
                            // eligible, -1 = there and at the tile counts where it was measured to pay (wave_preload_pays)
};

// Dynamic-LDS limit of a kernel: a per-DEVICE function attribute.  The one-process-all-GPUs mode launches the same
// kernel on several devices from several host threads, so "already set" is a bit per device ordinal (devices beyond
// 63 set it on every launch).
#include <atomic>
template <typename K>
inline hipError_t tp_allow_dynamic_lds(std::atomic<unsigned long long>& done_mask, K kernel, int bytes) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    const unsigned long long bit = (dev >= 0 && dev < 64) ? (1ull << dev) : 0ull;
    if (bit && (done_mask.load(std::memory_order_acquire) & bit)) return hipSuccess;
    e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e != hipSuccess) return e;
    if (bit) done_mask.fetch_or(bit, std::memory_order_release);
    return hipSuccess;
}

// Device-side view of one batch (all pointers are DEVICE pointers; optional ones may be null).
struct tp_kargs_t {
    const double* panel;
    const long long* start;
    const int* row_idx;
    const int* n_rows;
    const int* col_idx;
    const double* rf_adj;
    const double* hf_panel;
    const long long* hf_start;
    const int* hf_row_idx;
    const int* hf_count;
    const double* w0;
    const double* n0;
    const double* prefix; // optional (contiguous layout, no rf_adj): workspace of the shared Gram sums of the daily panel:
                          // the per-block Grams G[prefix_nblk][slot], filled by every launch before the window kernel (the
                          // register-tile path builds its tables without them unless shared_tables says otherwise: left unwritten)
    int prefix_nblk;      // whole TP_PREFIX_BLOCK_ROWS-row blocks of the panel
    int prefix_blk0;      // large-k path: the tables cover blocks prefix_blk0 .. prefix_blk0 + prefix_nblk - 1 (those of the
                          // sub-batch in flight; a whole-panel table at k = 1000 and 125,000 windows would be 102 GB); else 0
    // behind the block Grams: one table of block-window sums Q_L[b0] = G[b0] + .. + G[b0 + L - 1] per whole-block count
    // L that occurs among the batch's windows (at most TP_WINSUM_MAX_L)
    const double* winsum; // Q tables: [n_L][prefix_nblk][slot]
    int winsum_L[4];      // the block counts L (0 = unused entry)
    // large-k path, conjugate, contiguous intraday windows that advance by a fixed stride B (one day of bars): the whole
    // B-row blocks of every window come from block Grams of the intraday panel that the windows of ONE sub-batch share
    // (DESIGN.md section 4b).  Tables of the sub-batch in flight, rebuilt by every launch; null = every row through the MFMAs
    const double* hf_prefix;   // block Grams [hf_nblk][slot] of the raw intraday rows (ones in the border column)
    const double* hf_winsum;   // block-window sums [hf_nblk][slot]: Q[b] = G[b] + .. + G[b + hf_L - 1]
    long long hf_row0;         // intraday panel row where block 0 of these tables starts
    int hf_blk_rows, hf_nblk, hf_L;
    const double* rhs;    // optional [W x k]: replaces the border column before the factorisation
    const double* shift;  // optional [W x 2], Jeffreys only: (d, e) adds d I + e 1 1' to the matrix that is factorised
    double* weights;
    int* status;
    double* aux;
    double* out_rhs;      // optional [W x k]: the right-hand side (border column) each window was solved for
    long long* stamps;    // diagnostic builds only: [w_count x 8] s_memtime stamps per window
    double* dbg_S1;       // optional [k*k + k]: S1 (or J) and the right-hand side of window dbg_w
    long long dbg_w;
    int dbg_mode;         // 1 prior (S0 | c S0 w0), 2 canonical statistics (T | t), 3 posterior (S1 or J | rhs)
    double* out_post;     // optional [post_count x k x k] (tp_batch_keep_posterior): the k x k matrix window post_w0 + i
    long long post_w0, post_count;   // factorises (S1 or J, shift included), symmetric, full storage; written by every run
    long long w_first, w_count;
    int panel_ld, hf_ld;
    int panel_off32, hf_off32;   // bit 0: explicit-row windows, bit 1: contiguous windows may use 32-bit byte offsets (u24 x u24)
    int k, N, n_r, m, strategy;
    int phase_limit;      // diagnostic (TP_PHASE_LIMIT): 1 = stop after the Gram phases (outputs are then invalid)
    int center_rows;      // Jeffreys: 0 = J = T - t t'/N, 1 = divide by the window's row count instead, 2 = plain T
    int shared_tables;    // host-side only, the handle's option "shared_tables": how launch_one builds the Q tables: 1 = one
                          // kernel from the panel (posterior_shared_tables.hip), 0 = block_gram_kernel + tp_window_sums_kernel,
                          // -1 = the one kernel at the tile counts where it measured faster (tp_shared_tables_pays).  It sits
                          // in the 4 bytes of padding in front of gamma and not in tp_kopts_t: no kernel's argument offsets move
    double gamma;
    tp_kopts_t opts;      // host-side only: which kernels run this batch
    // (behind everything else: the kernels that do not read it keep their argument offsets)
    const double* winsum_zero;   // register-tile path: one all-zero slot behind the Q tables, for the windows of a sharing batch
                                 // that have no slot of their own (posterior_wave_impl.h, PRE); null: the batch does not qualify
};

static_assert(sizeof(tp_kargs_t) == 376 && offsetof(tp_kargs_t, gamma) == 344 && offsetof(tp_kargs_t, winsum_zero) == 368,
              "tp_kargs_t: a new member moved the kernels' argument offsets");

// shared_tables: what built the Q tables of the last register-tile launch: -1 = the batch has none, 0 = the pair of
// kernels, 1 = the one kernel (tp_get_option "last_shared_tables")
struct tp_launch_info_t { int grid, block, lds_bytes, ntile, shared_tables = -1; };

// Shared Gram prefixes of the register-tile path: aligned blocks of the staged chunk's rows (16; 32 with eight waves,
// NT >= 13); 16 rows on the tiled path.
#define TP_WINSUM_MAX_L 4           /* register-tile path: distinct whole-block counts per batch that get a table */
#define TP_WINSUM_RUN 16            /* block positions one thread of tp_window_sums_kernel serves (a group: posterior_fused.hip) */
#define TP_PREFIX_BLOCK_ROWS(nt) ((nt) <= 12 ? 16 : 32)
// doubles per table slot (one Gram of one block or block window: every upper-triangle tile, 4 registers x 64 lanes)
inline size_t tp_fused_slot_doubles(int k) { const int nt = (k + 1 + 15) / 16; return (size_t)(nt * (nt + 1) / 2) * 256; }
inline size_t tp_fused_prefix_bytes(int k, long long panel_rows, int n_L, int* nblk_out) {
    const int nt = (k + 1 + 15) / 16;
    const long long nblk = panel_rows / TP_PREFIX_BLOCK_ROWS(nt);
    if (nblk_out) *nblk_out = (int)nblk;
    return sizeof(double) * (size_t)nblk * (size_t)(1 + n_L) * tp_fused_slot_doubles(k);
}
// Q_L tables from the block Grams (posterior_fused.hip): elementwise, additions only, groups of TP_WINSUM_RUN positions
// abs0: absolute block index of table position 0 (groups are cut in absolute positions: posterior_fused.hip)
hipError_t tp_window_sums_launch(const double* G, double* Q, int nblk, size_t slot_doubles, const int* L, int n_L,
                                 hipStream_t stream, long long abs0 = 0);
// The same Q_L tables, bit for bit, in ONE kernel straight from the daily panel (posterior_shared_tables.hip): no block
// Grams in memory.  Register-tile path only (slot layout of block_gram_kernel, blocks of TP_PREFIX_BLOCK_ROWS rows, table
// position 0 = block 0).
hipError_t tp_shared_tables_launch(const double* panel, int ld, int k, double* Q, int nblk, const int* L, int n_L,
                                   hipStream_t stream);
// Tile counts at which the automatic choice (shared_tables = -1) takes the one kernel: where it measured faster than the
// pair on MI355X (profiles/r23_shared_tables_bench.txt)
bool tp_shared_tables_pays(int nt);

// which register-tile kernel runs a tile count: 0 = the multi-wave kernel (posterior_fused_impl.h), 1 = one wave per
// window (posterior_wave_impl.h), 2 = two / four waves per window (posterior_wave2_impl.h); `choice` =
// tp_kopts_t::wave_kernel >= 0 overrides the automatic pick (A/B measurements)
int tp_pick_wave_kernel(int nt, int choice);
// 0 / 1: a plain conjugate / Jeffreys batch (weights, statuses, aux only) - what the one-wave kernel is built for;
// 2: a batch with a matrix read-back, a custom right-hand side, tp_batch_keep_rhs, a shift or a non-default centring.
// Kept posterior matrices (out_post) do not count: such a batch runs on the kernel it would run on without them (the
// one- and two-wave kernels have instantiations with the store, tp_post_mode)
inline int wave_mode(const tp_kargs_t& a) {
    const bool plain = a.dbg_S1 == nullptr && a.rhs == nullptr && a.out_rhs == nullptr && a.shift == nullptr && a.center_rows == 0;
    return plain ? (a.strategy == 0 ? 0 : 1) : 2;
}

// instantiation of the one- / two-wave kernels for a plain mode m (0 / 1): m + 3 also stores the posterior matrices
inline int tp_post_mode(const tp_kargs_t& a, int m) { return a.out_post != nullptr ? m + 3 : m; }
// the kept matrix of window w (tp_batch_keep_posterior), or null when w is outside the kept range
__host__ __device__ inline double* tp_post_window(const tp_kargs_t& a, long long w) {
    const long long p = w - a.post_w0;
    return (a.out_post != nullptr && p >= 0 && p < a.post_count) ? a.out_post + p * (long long)a.k * a.k : nullptr;
}
// Stores of the kept matrices: written once, read by nobody on the device - non-temporal, so that they do not evict the
// panel rows the windows share from L2 / MALL.  (Against plain stores: not measured)
__device__ __forceinline__ void tp_post_store(double* p, double v) { __builtin_nontemporal_store(v, p); }

// register-tile fused kernel (posterior_fused.hip): k <= tp_fused_max_assets()
int tp_fused_max_assets(void);
hipError_t tp_fused_launch(const tp_kargs_t& a, int grid, hipStream_t stream, tp_launch_info_t* info,
                           int* want_occupancy);

// large-k tiled path (posterior_tiled.hip): k <= tp_tiled_max_assets().  The workspace holds the
// in-flight windows of one batch: arena [G][KP][KP], rinv [G][NSB][64][64], ybar [G][KP], zc [G][m],
// scal [G][8] (s, sqrt s, c, q0, n0), flags [G].
struct tp_tiled_ws_t {
    double* arena;
    double* rinv;
    double* ybar;
    double* zc;
    double* scal;
    int* flags;
    double* part;         // shared intraday sums: partial products S w0 per (window, row block, column block) [G][NS][NS][64]
    int KP, NS, NSB;
};
int tp_tiled_max_assets(void);
void tp_tiled_geometry(int k, int* KP, int* NS, int* NSB);
hipError_t tp_tiled_launch(const tp_kargs_t& a, const tp_tiled_ws_t& ws, hipStream_t stream, bool build_prefix);
// the two halves of tp_tiled_launch: the Gram stage leaves the bordered matrices in the arena (and stores out_rhs / out_post);
// the factor stage factorises and solves whatever a.w_count matrices the arena holds (entry e -> output slot a.w_first + e)
hipError_t tp_tiled_gram_launch(const tp_kargs_t& a, const tp_tiled_ws_t& ws, hipStream_t stream, bool build_prefix);
hipError_t tp_tiled_factor_launch(const tp_kargs_t& a, const tp_tiled_ws_t& ws, hipStream_t stream);
// the factor stage without its solve: the block steps alone, on a workspace of any geometry (KP, NS, NSB come from `ws`) -
// columns >= k of the pivot block rows come out forward-substituted (the tiled solve sweep back-substitutes them itself)
hipError_t tp_tiled_block_steps_launch(const tp_kargs_t& a, const tp_tiled_ws_t& ws, hipStream_t stream);
// bytes of the shared block Grams + n_L block-window tables of the daily panel in the tiled layout (16-row blocks)
size_t tp_tiled_prefix_bytes(int k, long long panel_rows, int n_L, int* nblk_out);
size_t tp_tiled_slot_doubles(int k);

// solve sweep (posterior_sweep.hip): one workgroup per (window, shift) of the windows [w_first, w_first + w_count), whose
// kept matrices lie in `post` (window w_first first).  All other arrays are indexed by the window's number in the batch.
#define TP_SWEEP_KMAX_RHS 16
struct tp_sweep_kargs_t {
    const double* post;         // [w_count x k x k] matrices M_w of this sub-range, symmetric, full storage
    const double* default_rhs;  // optional [W x k]: slot r = 0 (the window's own right-hand side)
    const double* rhs;          // optional [W x n_rhs x k]: the caller's columns, behind the default
    const double* shift;        // optional [W x S x 2] = (d, e): adds d I + e 1 1'
    double* x;                  // [W x S x R x k]
    int* status;                // [W x S]
    long long w_first, w_count;
    int k, S, R, n_rhs;
    double gamma;
};
int tp_sweep_max_k(void);
size_t tp_sweep_lds_bytes(int k, int R);
hipError_t tp_sweep_launch(const tp_sweep_kargs_t& a, hipStream_t stream);

// price front-end (returns_frontend.hip): out[i][c] = log(prices[num[i]][c] / prices[den[i]][c]), NaN -> 0
hipError_t tp_log_return_rows_launch(const double* prices, int ld, const int* num, const int* den, long long n_out,
                                     double* out, hipStream_t stream);
