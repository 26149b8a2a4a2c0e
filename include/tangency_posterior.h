/* tangency_posterior.h - C-ABI of libtangency.so: the MI355X (gfx950) implementation of the
 * rolling-window Bayesian tangency-portfolio posterior.
 *
 * The reference (vilnik/incorporating-different-sources) has no FFI: its boundary is the Python
 * module surface of src/portfolio_calculations.py.  The entry points below are what that module's
 * hot path binds through ctypes in this build (incorporating_different_sources_amd/_native.py);
 * each cites the reference interface it replaces as ref:LINE of src/portfolio_calculations.py.
 *
 * One "window" = one rebalancing date.  For every window w the library computes, in fp64,
 *
 *   X_w  (n_r x k)  rows of the daily excess-log-return panel            ref:31-62, 136-161
 *   T = X'X, t = X'1                                                     ref:163-245
 *   Y_w  (m x k)    rows of the intraday log-return panel                ref:310-314
 *   S0 = n0 * m/(m-1) * (Y-Ybar)'(Y-Ybar)                                ref:317-318, 333
 *   c  = 2 n0 / (a + sqrt(a^2 + 4 n0 w0'S0 w0)),  a = n0 + k + 2         ref:415-418
 *   S1 = S0 + T ;  w1 = S1^-1 (c S0 w0 + t) ;  n1 = n0 + N               ref:358, 485-489, 282
 *   weights = (n1 + k + 2) w1 / (n1 - w1'S1 w1) / gamma                  ref:572-575, 836
 * or, for TP_STRATEGY_JEFFREYS,
 *   weights = (T - t t'/N)^-1 t / gamma                                  ref:600-606, 849
 *
 * Everything is plain C: caller-allocated buffers, int return codes, no exceptions.  All arrays are
 * row-major with the asset index contiguous.  A handle owns one GPU, one HIP stream and (optionally)
 * one RCCL communicator; calls on one handle must be serialised by the caller.
 * There is NO CPU fallback: tp_create fails with TP_ERR_NO_DEVICE when no gfx950 device is usable.
 */
#ifndef TANGENCY_POSTERIOR_H
#define TANGENCY_POSTERIOR_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* return codes */
#define TP_OK 0
#define TP_ERR_INVALID (-1)     /* bad argument (the message is in tp_last_error) */
#define TP_ERR_NO_DEVICE (-2)   /* no usable HIP device */
#define TP_ERR_HIP (-3)         /* a HIP runtime call failed */
#define TP_ERR_UNSUPPORTED (-4) /* shape outside what the kernels cover (see tp_max_assets) */
#define TP_ERR_RCCL (-5)        /* an RCCL call failed */

/* weighting strategies on the path (ref:1012-1034 dispatch) */
#define TP_STRATEGY_CONJUGATE 0 /* calculate_conjugate_hf_mcm_portfolio, ref:819-836 */
#define TP_STRATEGY_JEFFREYS 1  /* calculate_jeffreys_portfolio,         ref:838-849 */

/* per-window status written to status[w] */
#define TP_STATUS_OK 0
#define TP_STATUS_NOT_PD 1    /* non-positive pivot: S1 (or J) is not positive definite (rank-deficient
                                 window; the reference returns finite garbage) */
#define TP_STATUS_NONFINITE 2 /* NaN/Inf in the weights (ref:492-494 raises ValueError) */
#define TP_STATUS_BAD_DENOM 3 /* n1 - w1'S1 w1 <= 0 (ref:573 has no guard, Appendix B-Q9) */
#define TP_STATUS_NO_CONVERGENCE 4 /* tp_batch_spectral_greyserman: the eigensolver reached TP_SPECTRAL_MAX_SWEEPS sweeps */

#define TP_AUX_STRIDE 8 /* doubles per window in `aux`: n0, n1, c, q0, q1, n1-q1, 0, 0 */

/* tp_params_t.flags */
#define TP_FLAG_CENTER_BY_ROWS 1 /* Jeffreys scatter T - t t'/n_w with n_w = the rows window w actually
                                   uses instead of N: (n_w - 1) x the sample covariance (ref:876, 917) */
#define TP_FLAG_NO_CENTER 2      /* Jeffreys strategy on the plain Gram matrix T = X'X (no - t t'/N term):
                                   (n-1) S + n xbar xbar' of ref:924 is exactly T */

#define TP_FLAG_NO_SHARED_GRAM 4  /* do not share Gram sums between overlapping windows (contiguous layout): every
                                   window pushes all its rows through the MFMAs, as the index layout always does */

typedef struct tp_handle_s* tp_handle_t;
typedef struct tp_batch_s* tp_batch_t;

/* The reference's portfolio_spec dict (src/portfolio_specs.py:80-90) reduced to what the path reads. */
typedef struct tp_params {
    int32_t k;        /* portfolio_spec["size"]            (ref:415, 572) */
    int32_t N;        /* portfolio_spec["rolling_window"]  (ref:265, 282, 600) */
    int32_t n_r;      /* max rows of excess returns per window (= N-1 without NaN drops, ref:60) */
    int32_t m;        /* max intraday returns per window (conjugate only; ref:314) */
    int32_t strategy; /* TP_STRATEGY_* */
    int32_t flags;    /* TP_FLAG_* */
    double gamma;     /* portfolio_spec["risk_aversion"]   (ref:836, 849) */
} tp_params_t;

/* Host-side description of W windows (all pointers are HOST pointers; optional ones may be NULL).
 * Window w reads
 *   daily rows   row_idx ? row_idx[w*n_r + r] : start[w] + r          for r < (n_rows ? n_rows[w] : n_r)
 *   asset column col_idx ? col_idx[w*k + j]   : j                      for j < k
 *   x[r][j] = panel[row*panel_ld + col] - (rf_adj ? rf_adj[w*n_r + r] : 0)     (ref:57)
 *   intraday rows hf_row_idx ? hf_row_idx[w*m + r] : hf_start[w] + r   for r < (hf_count ? hf_count[w] : m)
 */
typedef struct tp_inputs {
    const double* panel;       /* [panel_rows x panel_ld] daily log-return panel */
    int64_t panel_rows;
    int32_t panel_ld;
    int32_t hf_ld;
    const int64_t* start;      /* [W] first panel row of each window (contiguous mode) */
    const int32_t* row_idx;    /* optional [W x n_r] explicit panel rows (overrides start) */
    const int32_t* n_rows;     /* optional [W] rows actually used (<= n_r) */
    const int32_t* col_idx;    /* optional [W x k] panel columns of the k selected assets */
    const double* rf_adj;      /* optional [W x n_r] per-row risk-free adjustment, ref:48-57 */
    const double* hf_panel;    /* [hf_rows x hf_ld] intraday log-return panel (conjugate) */
    int64_t hf_rows;
    const int64_t* hf_start;   /* [W] */
    const int32_t* hf_row_idx; /* optional [W x m] */
    const int32_t* hf_count;   /* optional [W] intraday returns actually used (<= m, >= 2) */
    const double* w0;          /* [W x k] prior weights, ref:361-380 */
    const double* n0;          /* [W] prior strength, ref:247-267 */
    /* Optional price front-end (ref:31-62, 136-161, 299-314).  With `ret_num` given, `panel` holds PRICES
     * [panel_rows x panel_ld] and the library forms the log-return panel on the device,
     *     R[i][c] = log(P[ret_num[i]][c] / P[ret_den[i]][c])   for i < ret_rows   (NaN -> 0, +-inf -> +-DBL_MAX),
     * e.g. (i, i-1) for daily returns, (bin end, previous bin end) for weekly / monthly resampled windows and
     * (date, last complete bin end) for the running bin.  start / row_idx then address rows of R (and are
     * checked against ret_rows).  `hf_ret_num` does the same for the intraday panel.  Zero-initialise the
     * struct to leave the front-end off: the panels are then log-returns, as above. */
    const int32_t* ret_num;    /* optional [ret_rows] price row in the numerator */
    const int32_t* ret_den;    /* [ret_rows] price row in the denominator (required with ret_num) */
    int64_t ret_rows;
    const int32_t* hf_ret_num; /* optional [hf_ret_rows] */
    const int32_t* hf_ret_den;
    int64_t hf_ret_rows;
} tp_inputs_t;

const char* tp_version(void);
/* largest portfolio_spec["size"] the built kernels cover */
int tp_max_assets(void);
/* largest k the sweep kernels cover (tp_batch_solve_sweep, tp_batch_prior_sweep); at least 143, at most tp_max_assets() */
int tp_sweep_max_assets(void);
/* number of visible HIP devices (0 when there is none: tp_create will then fail) */
int tp_device_count(void);

/* Contexts.  tp_create binds device `device_id`, creates a stream and timing events.
 * Replaces: nothing in the reference (it has no device); corresponds to process start-up. */
int tp_create(int device_id, tp_handle_t* out);
/* Destroys the handle AND every batch of it that is still alive (their tp_batch_t become invalid).  Lifetime rule
 * for host languages with finalisers: whatever is still alive when the process exits is taken down by the library's
 * own exit handler (registered by the first tp_create, so it runs before the HIP / RCCL runtimes unload: batches
 * first, then the communicator, streams, events); tp_destroy / tp_batch_destroy calls that arrive after that -
 * from finalisers that run during interpreter shutdown - return TP_OK without touching the device or the handle. */
int tp_destroy(tp_handle_t h);
/* Tuning switches of a handle (A/B measurements, tests).  The environment variables of the same meaning
 * (TP_WAVE_KERNEL, TP_TILED_WAVE, TP_TILED_FUSE, TP_NO_SHARED_GRAM, TP_TILED_ARENA_GIB, TP_TILED_ARENA_MIB) are read
 * ONCE, in tp_create; afterwards only this call changes them - no launch reads the environment.
 *   "wave_kernel"      -1 automatic | 0 multi-wave register-tile kernel | 1 one-wave kernel | 2 two-wave kernel
 *   "tiled_wave"       -1 automatic | 0 four-wave Gram / diagonal-block kernels of the large-k path | 1 one wavefront per
 *                      super-tile / block (what automatic picks); any other value: TP_ERR_INVALID (in the
 *                      environment: automatic)
 *   "tiled_fuse"       -1 automatic | 0 / 1 three-kernel / fused left-looking update of the large-k path
 *   "wave_preload"     1 the one-wave kernel starts a window's accumulators from its shared table slot wherever the batch
 *                      qualifies (plain conjugate, contiguous layout with shared sums, k mod 16 <= 13) | -1 automatic: there,
 *                      at the sizes where that measured faster | 0 never (A/B measurements); any other value: TP_ERR_INVALID
 *   "shared_tables"    how a register-tile batch (k <= 239) with shared sums builds its block-window tables, every run:
 *                      1 one kernel straight from the daily panel | 0 the pair of kernels used before (block Grams to
 *                      memory, then their sums) | -1 automatic: the one kernel at the tile counts where it measured faster.
 *                      The tables are the same bit for bit; any other value: TP_ERR_INVALID.  No environment variable
 *   "no_shared_gram"   1 = as if every batch carried TP_FLAG_NO_SHARED_GRAM (takes effect at the next upload)
 *   "tiled_arena_gib" / "tiled_arena_mib"  in-flight arena of the large-k path (0: default)
 *   "hf_share_min_blocks"  large-k path, conjugate: intraday windows that advance by a fixed stride share the Grams of
 *                      their whole stride-long blocks from this many whole blocks per window on (default 6; takes effect
 *                      at the next upload; "no_shared_gram" switches the scheme off)
 *   "sweep_chunk_windows"  windows per sub-range of tp_batch_solve_sweep and tp_batch_prior_sweep (0 automatic: as many as
 *                      256 MiB of k x k matrices hold - the prior sweep keeps two per window and never exceeds that);
 *                      results do not depend on it
 * Replaces nothing in the reference. */
int tp_set_option(tp_handle_t h, const char* name, int value);
/* The current value of an option tp_set_option takes, and one read-only name: "last_shared_tables" = what built the
 * tables of the last tp_batch_run on the register-tile path: 1 the one kernel, 0 the pair, -1 the batch had none (or the
 * run was on the large-k path).  An unknown name: TP_ERR_INVALID. */
int tp_get_option(tp_handle_t h, const char* name, int* value);
const char* tp_last_error(tp_handle_t h); /* h may be NULL: last error of a failed tp_create */
int tp_device_info(tp_handle_t h, char* name, int name_len, int* compute_units, int* clock_mhz,
                   int64_t* hbm_bytes);

/* The price front-end on its own: out[i][c] = log(prices[num[i]][c] / prices[den[i]][c]) for i < n_out, c < ld
 * (NaN -> 0, +-inf -> +-DBL_MAX), host buffers in and out.  Replaces the np.log(prices / prices.shift(1)) of
 * ref:44 (daily or resampled prices) and ref:311 (intraday bars); tp_batch_upload runs the same kernel when
 * tp_inputs_t.ret_num is set, without the copy back. */
int tp_log_returns(tp_handle_t h, const double* prices, int64_t price_rows, int32_t ld, const int32_t* num,
                   const int32_t* den, int64_t n_out, double* out /* [n_out x ld] */);

/* A batch is W windows resident in HBM: inputs uploaded once, run any number of times.
 * Replaces the per-date loop body of Portfolio.update_portfolio -> calculate_portfolio_weights
 * (ref:1184 -> ref:941) for all rebalancing dates of a backtest at once. */
int tp_batch_create(tp_handle_t h, const tp_params_t* p, int64_t W, tp_batch_t* out);
int tp_batch_upload(tp_batch_t b, const tp_inputs_t* in);   /* H2D, synchronous */
/* The same upload queued on the handle's copy stream and not waited for: with the host arrays in page-locked
 * memory (tp_host_alloc) the copies of the NEXT batch run under the kernel of the current one (a backtest that
 * streams batches through tp_batch_run, ref:1232 loop over dates in chunks).  The host arrays must stay valid
 * until tp_batch_upload_wait returns (or the following tp_batch_run has been synchronised); the next tp_batch_run
 * of this batch waits for the copies on the device.  Validation of the index arrays still happens in the call. */
int tp_batch_upload_async(tp_batch_t b, const tp_inputs_t* in);
int tp_batch_upload_wait(tp_batch_t b);                     /* host wait for the queued copies; sets h2d_ms */
/* After an upload: the number of aligned row blocks of the daily panel whose Gram sums the windows of this batch share
 * (rolling windows in the contiguous layout); 0 when every window sums all its own rows. */
int tp_batch_shared_gram_blocks(tp_batch_t b);
/* After an upload, large-k path, conjugate: whole stride-long blocks of intraday rows per window whose Grams the windows
 * of a sub-batch share (0: every intraday row of every window goes through the MFMAs). */
int tp_batch_shared_intraday_blocks(tp_batch_t b);
/* How the Gram kernels form their load addresses for a panel of `panel_bytes` bytes with leading dimension `ld` (doubles)
 * whose windows have `rows_per_window` rows (n_r for the daily panel, m for the intraday one).  Needs no device.
 * Bit 0: windows with explicit rows use one 32-bit byte offset per row from the panel base (the panel is below 2^32
 * bytes and has fewer than 2^24 rows).  Bit 1: contiguous windows use 32-bit offsets from the window's first row
 * ((rows_per_window + 64) * ld * 8 < 2^32 and rows_per_window < 2^24).  Both clear when ld < 1 or 8 ld >= 2^24.  A clear bit: 64-bit addresses. */
int tp_addressing_flags(int64_t panel_bytes, int32_t ld, int32_t rows_per_window);
/* After an upload: the flag words above as the next launch of this batch will see them, for the daily panel and the
 * intraday panel (0 when the batch has none).  Either pointer may be NULL. */
int tp_batch_addressing(tp_batch_t b, int* panel_flags, int* hf_flags);
/* Page-locked host memory for panels and result arrays (hipHostMalloc): DMA at PCIe rate, asynchronous. */
int tp_host_alloc(void** out, int64_t bytes);
int tp_host_free(void* p);
/* Optional right-hand side [W x k] replacing the border column (t for Jeffreys, c S0 w0 + t for the
 * conjugate posterior) in every later tp_batch_run.  Jeffreys: the weights become (matrix)^-1 rhs / gamma.
 * Conjugate: rhs replaces c S0 w0 + t in w1 = S1^-1 rhs (ref:485-489) and the nu rescale of ref:572-575 still
 * applies: weights = (n1 + k + 2) w1 / (n1 - w1'S1 w1) / gamma, aux slots 4 and 5 (w1'S1 w1 and the denominator)
 * and TP_STATUS_BAD_DENOM follow that w1; the plain solve S1^-1 rhs / gamma is tp_batch_solve_sweep's.  NULL
 * restores the default.  Binds the V^-1 1 / V^-1 mu solves of calculate_jorion_portfolio (ref:880-891). */
int tp_batch_set_rhs(tp_batch_t b, const double* rhs);
/* Optional per-window shift [W x 2] = (d_w, e_w), Jeffreys strategy only: the matrix that is factorised
 * becomes J_w + d_w I + e_w 1 1' in every later tp_batch_run (NULL restores the default).  d_w >= 0,
 * e_w >= 0 keep it positive definite.  Binds the scale matrix D_h of calculate_greyserman_portfolio
 * (ref:924: eta_b S_h = eta_b/2 (I + 1 1'), kappa_h xi_b^2 1 1'), one window per posterior draw. */
int tp_batch_set_shift(tp_batch_t b, const double* shift);
int tp_batch_run(tp_batch_t b);                             /* async on the handle's stream; HIP-event timed */
/* Keep (on != 0) the right-hand side each window is solved for in every later tp_batch_run (default: t = X'1,
 * ref:222, resp. c S0 w0 + t, ref:489): tp_batch_download_rhs then copies out what the LAST run used.  It never
 * launches anything itself: without a run after tp_batch_keep_rhs it fails with TP_ERR_INVALID. */
int tp_batch_keep_rhs(tp_batch_t b, int on);
int tp_batch_download_rhs(tp_batch_t b, double* rhs_out /* [W x k] */);
/* Keep the k x k matrix each window of [w_begin, w_begin + w_count) factorises - S1 (ref:358) for the conjugate
 * strategy, J (ref:600-601) for Jeffreys, with a tp_batch_set_shift shift included: the same matrix
 * TP_MATRIX_POSTERIOR reads back - in every later tp_batch_run.  Written by the kernels of the run itself (no extra
 * launch on the register-tile path, and the same kernel as without it); w_count = 0 stops it.  Device memory:
 * w_count * k * k doubles, allocated in this call (TP_ERR_HIP names the byte count when that fails) and freed by
 * w_count = 0 or tp_batch_destroy.  A range outside [0, W) is TP_ERR_INVALID. */
int tp_batch_keep_posterior(tp_batch_t b, int64_t w_begin, int64_t w_count);
/* The matrices the LAST tp_batch_run kept; without a run after tp_batch_keep_posterior: TP_ERR_INVALID. */
int tp_batch_download_posterior(tp_batch_t b, double* M /* [w_count x k x k], symmetric, full storage */);
/* Solve sweep: many shifts and right-hand sides per window from ONE Gram pass.  With S = max(n_shift, 1) and
 * R = (default_rhs ? 1 : 0) + n_rhs, for every window w, shift s and right-hand side r
 *     x[w][s][r] = (M_w + d_ws I + e_ws 1 1')^-1 rhs_wr / gamma          (the / gamma is tp_batch_set_rhs's convention)
 * M_w is the matrix a plain tp_batch_run of this batch factorises: S1 (conjugate) or J (Jeffreys, with
 * TP_FLAG_CENTER_BY_ROWS / TP_FLAG_NO_CENTER honoured); a tp_batch_set_shift shift of the batch is NOT included, and
 * its tp_batch_set_rhs is not used.  With default_rhs != 0 slot r = 0 is the window's own right-hand side (t, or
 * c S0 w0 + t) and the caller's n_rhs columns follow.  shift == NULL (n_shift 0 or 1) is one unshifted solve; a shift
 * needs the Jeffreys strategy and finite d, e >= 0.  TP_ERR_INVALID: a shift on a conjugate batch, a negative or
 * non-finite d or e, R outside [1, TP_SWEEP_MAX_RHS], n_shift < 0, n_shift > 1 without shift, n_rhs > 0 without rhs, a
 * batch that was not uploaded.  TP_ERR_UNSUPPORTED: k > tp_sweep_max_assets().  TP_ERR_HIP: an allocation failed (the
 * message names the byte count).
 * How it runs: the windows go through in sub-ranges ("sweep_chunk_windows"; default: as many as 256 MiB of matrices
 * hold).  Per sub-range the batch's own run kernel stores M_w and the default right-hand side (the machinery of
 * tp_batch_keep_posterior / tp_batch_keep_rhs; never with the shared block sums, so M_w depends on the window's rows
 * alone), then one workgroup per (window, shift) factorises once and solves all R columns.  A (window, shift) result does
 * not depend on W, S, the window's position or the sub-ranges.  Device memory: W x S x R x k doubles of solutions, four
 * [W x k]-sized arrays and the sub-range's matrices; kept until tp_batch_destroy.
 * The call copies shift and rhs to the device (no host pointer is kept) and queues the kernels on the handle's stream
 * without waiting for THEM.  Unlike tp_batch_run it does wait, on entry, for whatever was queued on the handle's stream
 * before it (an earlier run or sweep) and for its own two copies.  kernel_ms of tp_last_timing covers Gram passes and
 * solves; between tp_region_begin and tp_region_end a sweep counts as one step of tp_region_steps.  A gather requested
 * by tp_batch_gather_async is put on its stream at the end of the call, as at the end of a tp_batch_run; it carries the
 * results of the run it was requested for.  A later tp_batch_upload_async of the batch waits for the sweep's kernels.  It leaves the batch alone: its
 * set_rhs / set_shift / keep_rhs / keep_posterior settings stay, and tp_batch_download / tp_batch_download_rhs /
 * tp_batch_download_posterior return what they returned before.
 * Binds (T + eta_b/2 I)^-1 [t, 1] over the posterior draws of calculate_greyserman_portfolio (ref:924) and the
 * V^-1 [mu, 1] pair of calculate_jorion_portfolio (ref:880-891). */
#define TP_SWEEP_MAX_RHS 16
int tp_batch_solve_sweep(tp_batch_t b, int32_t n_shift, const double* shift /* [W x n_shift x 2] or NULL */,
                         int32_t n_rhs, const double* rhs /* [W x n_rhs x k] or NULL */, int32_t default_rhs);
/* Solve sweep for k > tp_sweep_max_assets(): the same definition of M_w, arguments, validation and result buffers as
 * tp_batch_solve_sweep - download with tp_batch_download_sweep / tp_batch_download_sweep_rhs - on the large-k tiled pipeline.
 * TP_ERR_UNSUPPORTED: k <= tp_sweep_max_assets() (tp_batch_solve_sweep serves those sizes and keeps refusing the larger
 * ones), or k + R > tp_max_assets() + 1 (the arena side would exceed 2048).
 * How it runs: per sub-range of windows ("sweep_chunk_windows"; one k x k matrix per window inside 256 MiB, at least one
 * window) the batch's own tiled Gram kernels - its real strategy, without its set_rhs / set_shift and never with the shared
 * daily or intraday block sums, so M_w depends on the window's rows alone - store M_w and the default right-hand side.  Then
 * every (window, shift) pair takes one entry of a tiled workspace the SWEEP owns, whose arena side is
 * KP = 64 ceil((k + R)/64): a fill pass writes M_w + d I + e 1 1' into the k x k corner, the R right-hand sides into columns
 * k .. k+R-1 and zeros elsewhere; the block steps of tp_batch_run's tiled factorisation, which take their geometry from the
 * workspace and carry every column >= k of a pivot block row along, factorise the entry ONCE and forward-substitute all R
 * columns; a back substitution of the sweep's own solves them in groups of up to four columns.  Entries go through in groups
 * of the workspace's capacity.  A (window, shift) result depends on the window's rows, its own shift and right-hand sides, k
 * and R only - not on W, S, the positions, the sub-ranges or the size of the workspace.
 * Statuses: TP_STATUS_NOT_PD is the tiled run's rule, a pivot that is not > 0 (a NaN in the window's rows ends here, for
 * every shift of that window), and a pivot no larger than k 2^-52 times its own shifted diagonal element (an exactly repeated
 * column: rounding noise of either sign); TP_STATUS_NONFINITE: NaN / Inf in any of the R solutions.
 * Streams, timing (one HIP-event pair: one step of tp_region_steps, one kernel_ms over Gram passes, fills, factorisations and
 * solves), the gather hand-over and what the call leaves alone are as for tp_batch_solve_sweep, tp_last_launch included; it
 * waits, on entry, for whatever was queued on the handle's stream.
 * Device memory: that of tp_batch_solve_sweep without its three Gram-pass outputs, plus the batch's tiled run workspace as
 * tp_batch_run sizes it (NOT grown or re-shaped: it stays what later runs need) and the sweep's workspace of
 * 8 (KP^2 + 4096 ceil(k/64)) + 4 bytes per entry.  The entry count follows the run workspace's budget rule - 32 GiB, never
 * more than a third of the free memory, "tiled_arena_gib" / "tiled_arena_mib" override it - capped at the (window, shift)
 * pairs of one sub-range and at 65,535 (k = 500, R = 2: 2.4 MB per entry, 32 dates x 1000 shifts go through about 14,500 entries
 * at a time).  It is kept, like the other sweep buffers, until tp_batch_destroy. */
int tp_batch_solve_sweep_tiled(tp_batch_t b, int32_t n_shift, const double* shift /* [W x n_shift x 2] or NULL */,
                               int32_t n_rhs, const double* rhs /* [W x n_rhs x k] or NULL */, int32_t default_rhs);
/* Waits for the sweep (of either kind) and copies out x [W x S x R x k] and status [W x S] (TP_STATUS_OK, TP_STATUS_NOT_PD:
 * a pivot <= 0, TP_STATUS_NONFINITE: NaN / Inf in any of the R solutions); either may be NULL.  Without a sweep before it:
 * TP_ERR_INVALID. */
int tp_batch_download_sweep(tp_batch_t b, double* x, int32_t* status);
/* The default right-hand sides [W x k] (t, or c S0 w0 + t) the Gram pass of the last sweep formed, whether or not the
 * sweep solved for them (tp_batch_download_rhs keeps answering for the last tp_batch_run).  Waits like
 * tp_batch_download_sweep; without a sweep before it: TP_ERR_INVALID. */
int tp_batch_download_sweep_rhs(tp_batch_t b, double* rhs_out);
/* Sweep finish: the Greyserman (ref:928-931) or Jorion (ref:880-893) weights from the solutions the batch's LAST solve sweep
 * of either kind left on the device - no download of the W x S x 2 x k solutions; the results [W x k] stay on the device, where
 * tp_replay_run_batch reads them (TP_REPLAY_SRC_SWEEP_FINISH).  The sweep must have had R = 2: default_rhs (slot 0, u_t = M^-1 t)
 * and ONE caller column (slot 1, u_one), which MUST be the ones vector - the call cannot see that it is.  The batch must have
 * been created with gamma = 1 (the sweep divides by the batch's gamma; the finish takes `gamma` itself).
 * Definitions, all in double, ONE rounding per operation, in this order.  For window w and shift s, with u_one, u_t the two
 * solution rows, t the sweep's default right-hand side (tp_batch_download_sweep_rhs), N = k:
 *   s1 = sum_j u_one_j,  s2 = sum_j u_t_j,  s3 = sum_j fl(t_j u_t_j): lane l of a wavefront adds its columns l, l + 64, ... in
 *     ascending order starting from 0, then the 64 partials go through a fixed tree (rotations by 8, 4, 2, 1 inside each row of
 *     16 lanes, then (r0 + r1) + (r2 + r3) over the four rows).
 *   TP_FINISH_GREYSERMAN, with n = n[w], kappa = kappa[w], (xi, eta) = hyper[w][s]:
 *     beta = eta / 2 + kappa (xi xi);  K11 = 1 / beta + s1;  K12 = s2 - (kappa xi) / beta;
 *     K22 = (s3 - n) - (kappa eta) / (2 beta);  det = K11 K22 - K12 K12;
 *     c = ((1 / gamma) ((N + n) + 1)) (1 - 1 / n);  cA = c (K12 / det);  cB = c (K11 / det);
 *     term_sj = cA u_one_sj - cB u_t_sj.
 *   TP_FINISH_JORION (S = 1), with T = n[w]:
 *     kJ = (((T - N) - 2) (T - 1)) / T;  s_bb = kJ s1;  s_ab = (kJ s2) / T;  s_aa = (kJ s3) / (T T);  mu_g = s_ab / s_bb;
 *     q = (s_aa - (2 mu_g) s_ab) + (mu_g mu_g) s_bb;  lam = (N + 2) / q;  v = (N + 2) / ((N + 2) + T q);
 *     alpha = 1 + 1 / (T + lam);  beta = (lam / (T ((T + 1) + lam))) / s_bb;  g = (1 - v) s_ab + (v mu_g) s_bb;
 *     cT = (((1 - v) kJ) / T) / alpha;  cO = ((v mu_g) kJ) / alpha;  cS = (((beta / (alpha alpha)) kJ) g) / (1 + (beta / alpha) s_bb);
 *     term_sj = ((cT u_t_j + cO u_one_j) - cS u_one_j) / gamma.
 *   weights[w][j] = (sum over the groups of TP_FINISH_DRAWS_PER_WAVE consecutive shifts, in ascending order, of (the group's terms
 *     added in ascending s starting from 0)) / S.  The grouping and every order depend on (k, S) only: a window's weights are the
 *     same bit for bit whatever W, its position, or the sub-ranges of the sweep that fed it, and from run to run.
 * status[w]: the first status of the sweep's shifts s = 0, 1, ... of the window that is not TP_STATUS_OK - the weights row is
 * then NaN -; else TP_STATUS_NONFINITE when a weight of the row is not finite (beta = 0, det = 0, q = 0 end here); else
 * TP_STATUS_OK.  aux[w][s] = (s1, s2, s3, det) - Jorion: (s1, s2, s3, q) -, NaN for a shift the sweep flagged.
 * TP_ERR_INVALID, all checked before anything is waited for, uploaded or queued (a refused call leaves the last finish in place):
 * an unknown mode; no solve sweep yet; a last sweep that was not R = 2 with default_rhs; a batch gamma other than 1;
 * TP_FINISH_JORION with S != 1; a NULL n - TP_FINISH_GREYSERMAN: kappa, hyper - with W > 0; a non-finite n, kappa, xi or eta; a
 * gamma that is 0 or not finite.  kappa and hyper are not read by TP_FINISH_JORION and may be NULL.
 * The call waits on entry for whatever is queued on the handle's stream - the sweep ends here -, uploads n, kappa and hyper (HOST
 * pointers, not kept) and queues two launches inside one timed span without waiting for them: kernel_ms, one step of
 * tp_region_steps; tp_last_launch keeps describing tp_batch_run.  The sweep's solutions are not written.  Buffers (the results,
 * W x ceil(S / TP_FINISH_DRAWS_PER_WAVE) x k doubles of partial sums and the uploaded scalars) are kept until tp_batch_destroy.
 * A later tp_batch_solve_sweep[_tiled] that gets as far as its drain replaces the solutions: the finish is then no longer valid,
 * tp_batch_download_sweep_finish and TP_REPLAY_SRC_SWEEP_FINISH are refused (TP_ERR_INVALID, the message says why). */
#define TP_FINISH_GREYSERMAN 0
#define TP_FINISH_JORION     1
#define TP_FINISH_DRAWS_PER_WAVE 16
int tp_batch_sweep_finish(tp_batch_t b, int mode, double gamma, const double* n /* [W] */,
                          const double* kappa /* [W], Greyserman */, const double* hyper /* [W x S x 2] = (xi, eta), Greyserman */);
/* Waits for the finish and copies out weights [W x k], status [W] and aux [W x S x 4]; each may be NULL. */
int tp_batch_download_sweep_finish(tp_batch_t b, double* weights /* [W x k] */, int32_t* status /* [W] */, double* aux /* [W x S x 4] */);
/* Spectral ridge sweep: the Greyserman weights (ref:928-931) of n_shift ridge draws per window from ONE eigendecomposition of
 * the window's matrix instead of one factorisation per draw - and without the W x S x 2 x k solutions of a solve sweep.  For a
 * Jeffreys batch created with gamma = 1, k <= tp_sweep_max_assets().  M_w and t_w are what the solve sweep's Gram pass stores
 * (tp_batch_solve_sweep; the shared block sums are never used: M_w depends on the window's rows alone).  Every shift
 * d_s = eta_s / 2 is a multiple of the identity, so with M_w = V diag(lambda) V':  (M_w + d_s I)^-1 b = V diag(1 / (lambda_j + d_s)) V'b.
 * Definitions, all in double, ONE rounding per operation, in this order.
 * 1. Eigendecomposition (one 256-thread workgroup per window): two-sided cyclic Jacobi on the lower triangle of M_w.  A sweep is
 *    the m - 1 rounds of a round-robin tournament over m = 2 ceil(k / 2) players: in round r player m - 1 meets player r, and
 *    for u = 1 .. m / 2 - 1 player (r + u) mod (m - 1) meets player (r - u) mod (m - 1); (p, q) = the smaller and the larger of
 *    the two, a pair with q = k (k odd) sits out.  A pair is SKIPPED when |a_pq| <= 2^-53 max(sqrt(|a_pp a_qq|), a_max), a_max =
 *    max_i |M_ii| of the input.  Otherwise theta = (a_qq - a_pp) / (2 a_pq), tt = sign(theta) / (|theta| + sqrt(theta theta + 1))
 *    (sign(0) = +1), c = 1 / sqrt(tt tt + 1), s = tt c;  a_pp -= tt a_pq, a_qq += tt a_pq, a_pq = 0 exactly.  All rotations of a
 *    round are formed from the matrix as the round found it and applied together: an element (x, y) with x in pair u, y in pair
 *    v, u < v, takes pair v's rotation as a column ((e_p, e_q) <- (c e_p - s e_q, s e_p + c e_q)) and then pair u's as a row.
 *    The columns of V (from the identity) and the two rows t^ = V't (from t_w) and o^ = V'1 (from the ones vector) take the
 *    column rotation.  It ends after the first sweep without a rotation: lambda_j = a_jj, not sorted.  sweeps[w] counts that
 *    last sweep too.  After TP_SPECTRAL_MAX_SWEEPS sweeps with rotations: TP_STATUS_NO_CONVERGENCE (never reported as NOT_PD).
 *    A non-finite element of M_w or t_w: TP_STATUS_NONFINITE before the first sweep, no rotation.
 * 2. Per shift s, with d = eta / 2 and N = k:  r_j = 1 / (lambda_j + d),  uo_j = r_j o^_j,  ut_j = r_j t^_j,
 *      s1 = sum_j fl(uo_j o^_j),  s2 = sum_j fl(uo_j t^_j),  s3 = sum_j fl(ut_j t^_j): the lane-local order and the fixed 64-lane
 *    tree of tp_batch_sweep_finish (lane l owns j = l, l + 64, l + 128).  Then beta, K11, K12, K22, det, c, cA, cB exactly as
 *    TP_FINISH_GREYSERMAN defines them, and term_sj = cA uo_j - cB ut_j.  A shift with
 *      min_j lambda_j + d <= (k 2^-52) (max_j lambda_j + d)
 *    is TP_STATUS_NOT_PD (the tiled sweep's pivot rule, stated on eigenvalues) and contributes nothing.
 * 3. w^_j = (sum over the groups of TP_FINISH_DRAWS_PER_WAVE consecutive shifts, in ascending order, of (the group's terms added
 *    in ascending s starting from 0)) / S;  weights[w][i] = sum_j fl(V_ij w^_j), j ascending from 0.
 * The grouping and every order depend on (k, S) only: a window's weights are the same bit for bit whatever W, its position and
 * the sub-ranges, and from run to run.
 * status[w]: the eigensolver's status when it is not TP_STATUS_OK; else the first shift s = 0, 1, ... that is TP_STATUS_NOT_PD -
 * in both cases the weights row is NaN -; else TP_STATUS_NONFINITE when a weight of the row is not finite (beta = 0, det = 0 end
 * here); else TP_STATUS_OK.  aux[w][s] = (s1, s2, s3, det), NaN for a flagged shift.
 * TP_ERR_INVALID, all checked before anything is waited for, uploaded or queued (a refused call leaves the last result in
 * place): a batch that was not uploaded; not a Jeffreys batch; a batch gamma other than 1; n_shift < 1; a NULL n, kappa or hyper
 * with W > 0; a non-finite n, kappa, xi or eta; eta < 0; a gamma that is 0 or not finite.  TP_ERR_UNSUPPORTED:
 * k > tp_sweep_max_assets().  TP_ERR_HIP: an allocation failed - with keep_vectors != 0 the call keeps V of all W windows
 * (W k k doubles, allocated in the call; the message names the byte count); otherwise V lives per sub-range only.
 * The call waits on entry like tp_batch_solve_sweep (same gather hand-over), copies n, kappa and hyper (HOST pointers, not kept)
 * and queues, per sub-range of windows ("sweep_chunk_windows"), the Gram pass and three launches inside one timed span without
 * waiting for them: kernel_ms, one step of tp_region_steps; tp_last_launch keeps describing tp_batch_run.  It has buffers of its
 * own, kept until tp_batch_destroy: runs, solve sweeps and an earlier tp_batch_sweep_finish keep their results. */
#define TP_SPECTRAL_MAX_SWEEPS 32
int tp_batch_spectral_greyserman(tp_batch_t b, int32_t n_shift, double gamma, const double* n /* [W] */,
                                 const double* kappa /* [W] */, const double* hyper /* [W x S x 2] = (xi, eta) */,
                                 int32_t keep_vectors);
/* Waits for the spectral sweep and copies out weights [W x k], status [W], aux [W x S x 4] = (s1, s2, s3, det), the eigenvalues
 * lambda [W x k], the sweep counts [W] and the eigenvectors V [W x k x k] (column-major per window: V_ij at [w][j][i]); each may
 * be NULL.  V needs keep_vectors != 0 in the call (else TP_ERR_INVALID), as does a call before any spectral sweep. */
int tp_batch_download_spectral(tp_batch_t b, double* weights /* [W x k] */, int32_t* status /* [W] */,
                               double* aux /* [W x S x 4] */, double* lambda /* [W x k] */, int32_t* sweeps /* [W] */,
                               double* V /* [W x k x k], needs keep_vectors */);
/* Prior sweep: many conjugate priors (n0, w0) per window from ONE pair of Grams - a grid of conjugate specs over the same
 * rebalancing dates (VIX / EPU x vw / ew x mcm_scaling, ref:247-267, 361-380) without a replica of every window per spec.
 * With C = sum (y - ybar)(y - ybar)' the centred intraday scatter of window w, T = X'X, t = X'1, m the window's own
 * intraday row count (hf_count[w] where given) and, for prior p, a = n0_wp m/(m-1):
 *     S1 = a C + T ;  q0 = a w0_wp'C w0_wp ;  c = 2 n0_wp / (g + sqrt(g^2 + 4 n0_wp q0)),  g = n0_wp + k + 2   (ref:333, 358, 415-418)
 *     w1 = S1^-1 (c a C w0_wp + t) ;  n1 = n0_wp + N ;  weights[w][p] = (n1 + k + 2) w1 / (n1 - w1'S1 w1) / gamma   (ref:489, 572-575, 836)
 * i.e. what tp_batch_run returns for the window with (w0_wp, n0_wp) uploaded (not bit for bit: the factorisation differs).
 * The batch's own uploaded w0 / n0 are not used, nor its tp_batch_set_rhs.  TP_ERR_INVALID: a Jeffreys batch, n_prior < 1,
 * n0 or w0 NULL, an n0 that is not finite and > 0, a non-finite w0, a batch that was not uploaded.  TP_ERR_UNSUPPORTED:
 * k > tp_sweep_max_assets() (also: index-layout windows of more than about 10,000 rows).  TP_ERR_HIP: an allocation failed
 * (the message names the byte count).
 * How it runs: the windows go through in sub-ranges that hold TWO k x k matrices per window ("sweep_chunk_windows";
 * default and upper bound: as many as 256 MiB hold).  Per sub-range one Gram pass - one wavefront per window, every row
 * through the MFMAs, never the shared block sums, so C, T and t depend on the window's rows alone - stores C (unscaled), T
 * and t; then one workgroup per (window, prior) forms a C + T and C w0 in one pass, factorises in LDS and solves.  A
 * (window, prior) result does not depend on W, n_prior, the prior's or the window's position or the sub-ranges.  Device
 * memory: W x n_prior x (2 k + 9) doubles of priors and results, [W x k] of t and the sub-range's matrices; kept until
 * tp_batch_destroy.
 * The call copies n0 and w0 to the device (no host pointer is kept) and queues the kernels on the handle's stream without
 * waiting for THEM.  Like tp_batch_solve_sweep it waits, on entry, for whatever was queued on the handle's stream before it
 * and for its own two copies.  kernel_ms of tp_last_timing covers Gram passes and solves (one HIP-event pair); between
 * tp_region_begin and tp_region_end a prior sweep counts as one step of tp_region_steps.  A gather requested by
 * tp_batch_gather_async is put on its stream at the end of the call, as at the end of a tp_batch_run.  It leaves the batch
 * alone: its set_rhs / set_shift / keep_rhs / keep_posterior settings stay, tp_batch_download / _rhs / _posterior /
 * _sweep return what they returned before, and tp_last_launch keeps describing the last tp_batch_run. */
int tp_batch_prior_sweep(tp_batch_t b, int32_t n_prior, const double* n0 /* [W x n_prior] */,
                         const double* w0 /* [W x n_prior x k] */);
/* Prior sweep for k > tp_sweep_max_assets() (up to tp_max_assets()): the same definition, arguments, validation and result
 * buffers as tp_batch_prior_sweep - download with tp_batch_download_prior_sweep - on the large-k tiled pipeline.
 * TP_ERR_UNSUPPORTED: k <= tp_sweep_max_assets() (tp_batch_prior_sweep serves those sizes).
 * How it runs: per sub-range of windows ("sweep_chunk_windows"; two k x k matrices per window inside 256 MiB, at least one
 * window) the batch's own tiled Gram kernels run twice, steered by their arguments - over the daily rows for T = X'X and
 * t = X'1, over the intraday rows for C - never with the shared block sums.  Then every (window, prior) pair takes one slot
 * of the batch's tiled workspace ("tiled_arena_gib" / "tiled_arena_mib"), in groups of as many pairs as it holds windows: one
 * pass forms a C + T, t and the pieces of a C w0 from the two stored matrices, a second one q0, c and the right-hand side, and
 * the tiled factorisation and solve of tp_batch_run do the rest.  A (window, prior) result depends on the window's rows, its
 * own prior and k only - not on W, n_prior, the positions, the sub-ranges or the size of the workspace.
 * CENTRING: C = Y'Y - (Y'1)(Y'1)'/m is centred through the RAW moments, not through a row of the window as the scatter of
 * tp_batch_run and tp_batch_prior_sweep is.  For returns - a mean far below the spread - the two agree to rounding; under a
 * large common offset of the intraday panel (|mean| >> spread) the raw-moment form loses the digits the offset takes.
 * Statuses are those of tp_batch_run on the large-k path: TP_STATUS_NOT_PD is a pivot that is not > 0 (no relative floor).
 * Streams, timing (one step of tp_region_steps, one kernel_ms), the gather hand-over and what the call leaves alone are as
 * for tp_batch_prior_sweep; it waits, on entry, for whatever was queued on the handle's stream.  Device memory: that of
 * tp_batch_prior_sweep plus the batch's tiled workspace and 64 NS^2 doubles per slot of it (NS = ceil((k+1)/64)).  The call
 * GROWS that workspace to min(W, sub-range) x n_prior slots where the arena budget allows - n_prior times what tp_batch_run
 * alone needs for those windows (k = 500, W = 256, n_prior = 16: about 10 GB against 0.6 GB) - and it stays that large, also
 * for later tp_batch_run calls, until tp_batch_destroy; "tiled_arena_gib" / "tiled_arena_mib" cap it. */
int tp_batch_prior_sweep_tiled(tp_batch_t b, int32_t n_prior, const double* n0 /* [W x n_prior] */,
                               const double* w0 /* [W x n_prior x k] */);
/* Waits for the prior sweep and copies out weights [W x n_prior x k], status [W x n_prior] (TP_STATUS_OK, TP_STATUS_NOT_PD:
 * a pivot <= 0 or no larger than k 2^-52 times its diagonal element of S1, i.e. lost to rounding; TP_STATUS_NONFINITE;
 * TP_STATUS_BAD_DENOM: n1 - w1'S1 w1 <= 0) and aux [W x n_prior x TP_AUX_STRIDE] (the
 * slots of tp_batch_download's aux); each may be NULL.  Without a prior sweep (of either kind) before it:
 * TP_ERR_INVALID. */
int tp_batch_download_prior_sweep(tp_batch_t b, double* weights, int32_t* status, double* aux);
/* Size sweep: n_size nested universes per window - the first sizes[0] < sizes[1] < ... <= k columns of the batch's universe -
 * from ONE pair of Grams and ONE factorisation per (window, prior): the `sizes` axis of a spec grid (ref:247-267) without a
 * pack, an upload and a batch per size.  It rests on the columns being ordered so that the smaller universe IS a prefix of the
 * larger one (select_universe returns the largest caps in descending order); the caller vouches for that - and for the
 * windows' rows being those the smaller universe would have had (batch.pack_windows_nested checks both).
 * Conjugate batch, prior p, size s with k_s = sizes[s]; C, T, t, m and a = n0_wp m/(m-1) as in tp_batch_prior_sweep:
 *     S1 = (a C + T)[:k_s,:k_s] ;  v = C[:k_s,:k_s] w0_wps[:k_s] ;  q0 = a w0_wps'v
 *     c = 2 n0_wp / (g + sqrt(g^2 + 4 n0_wp q0)),  g = n0_wp + k_s + 2 ;  w1 = S1^-1 (c a v + t[:k_s]) ;  n1 = n0_wp + N
 *     weights[w][p][s][:k_s] = (n1 + k_s + 2) w1 / (n1 - w1'S1 w1) / gamma ,   weights[w][p][s][k_s:] = 0
 * i.e. what tp_batch_run returns for a batch of size k_s over the prefix columns with (w0_wps, n0_wp) uploaded (not bit for
 * bit: the factorisation differs).  Only the first k_s entries of a w0 vector are read; the rest may hold anything.
 * Jeffreys batch: n_prior = 0, n0 = w0 = NULL, the outputs have P = 1: weights[w][0][s][:k_s] = M[:k_s,:k_s]^-1 t[:k_s] / gamma
 * with M = T - t t'/N or the form TP_FLAG_CENTER_BY_ROWS / TP_FLAG_NO_CENTER selects.
 * The batch's own uploaded w0 / n0 are not used, nor its tp_batch_set_rhs / tp_batch_set_shift.
 * TP_ERR_INVALID: a batch that was not uploaded; n_size outside [1, TP_SWEEP_MAX_RHS]; sizes NULL or not strictly increasing
 * within [1, k]; conjugate: n_prior < 1, n0 or w0 NULL, an n0 that is not finite and > 0, a non-finite w0 inside a prefix;
 * Jeffreys: n_prior != 0 or a non-NULL n0 / w0.  TP_ERR_UNSUPPORTED: k > tp_sweep_max_assets() (also, conjugate: index-layout
 * windows of more than about 10,000 rows).  TP_ERR_HIP: an allocation failed (the message names the byte count).
 * How it runs: sub-ranges of windows as in tp_batch_prior_sweep ("sweep_chunk_windows").  Per sub-range the Gram pass of the
 * prior sweep stores C, T and t (Jeffreys: the batch's own run kernel keeps M and t - it reads the daily inputs only); then one
 * workgroup per (window, prior) forms the lower triangle at k with one extra row per size, factorises it once in LDS and
 * back-substitutes every size over its own prefix.  The leading block of the factor is the factor of the leading block: a
 * size's result depends on the window's rows, its prior, k_s and k only - not on the other sizes, W, n_prior, the positions or
 * the sub-ranges.  A column at or beyond k_s - a duplicate, a zero column, a NaN - does not reach size s.
 * Device memory: W x P x n_size x (2 k + 9) doubles of priors and results, [W x k] of t and the sub-range's matrices; kept
 * until tp_batch_destroy.  Streams, the entry drain, timing (kernel_ms covers Gram passes and solves; one step of
 * tp_region_steps), the gather hand-over and what the call leaves alone are as for tp_batch_prior_sweep; in addition
 * tp_batch_download_prior_sweep returns what it returned before. */
int tp_batch_size_sweep(tp_batch_t b, int32_t n_size, const int32_t* sizes /* [n_size] */,
                        int32_t n_prior, const double* n0 /* [W x n_prior] */,
                        const double* w0 /* [W x n_prior x n_size x k] */);
/* tp_batch_size_sweep above tp_sweep_max_assets(), on the large-k tiled pipeline: the same definition, arguments, validation
 * and result buffers (tp_batch_download_size_sweep serves both calls), every (window, prior) factorised ONCE at k by the tiled
 * MFMA factorisation with the n_size right-hand sides riding along as columns k .. k+n_size-1 of the arena, then one prefix
 * back substitution per size.  Individual sizes may be anything within [1, k], sizes <= tp_sweep_max_assets() included.
 * TP_ERR_UNSUPPORTED: k <= tp_sweep_max_assets() (tp_batch_size_sweep serves those); k + n_size > tp_max_assets() + 1.
 * How it runs: per sub-range of windows the batch's own tiled Gram stage stores the matrices - conjugate: twice, steered by its
 * arguments, as in tp_batch_prior_sweep_tiled, so C is RAW-MOMENT centred (exact to rounding for returns, it loses digits under
 * a large common offset of the intraday panel); Jeffreys: once, the batch's real strategy and centring flag - never from the
 * shared daily or intraday sums.  The (window, prior) entries live in the tiled solve sweep's own workspace at R = n_size,
 * KP = 64 ceil((k+n_size)/64): the batch's run workspace is neither grown nor re-shaped.
 * Prefix isolation differs from tp_batch_size_sweep in one case.  A FINITE degenerate column j (a duplicate, a zero column)
 * leaves every size k_s <= j intact; the sizes beyond it are TP_STATUS_NOT_PD.  A NON-FINITE column j leaves the sizes
 * k_s <= 64 floor(j/64) intact; the sizes in (64 floor(j/64), j] may come back flagged (TP_STATUS_NONFINITE or _NOT_PD) - the
 * block steps multiply whole 64-row blocks with MFMAs, where a structural zero times a NaN is a NaN - and the sizes > j are
 * flagged.  No size is TP_STATUS_OK with numbers that are not its own.
 * A (window, prior, size) result does not depend on W, n_prior, the window's position, the sub-ranges or the arena's size;
 * across different size lists it is promised to the solve's rounding only (n_size sets the arena's side).
 * Device memory: that of tp_batch_size_sweep (no Gram-pass outputs) plus, per entry of the sweep's workspace,
 * KP^2 + 4096 ceil(k/64) doubles and, conjugate, 64 n_size ceil(k/64)^2 doubles of prior products - as many entries as the
 * arena budget allows ("tiled_arena_gib" / "tiled_arena_mib"), shared with tp_batch_solve_sweep_tiled, whose downloads are
 * left alone.  Streams, the entry drain, timing and the gather hand-over are as for tp_batch_size_sweep. */
int tp_batch_size_sweep_tiled(tp_batch_t b, int32_t n_size, const int32_t* sizes /* [n_size] */,
                              int32_t n_prior, const double* n0 /* [W x n_prior] */,
                              const double* w0 /* [W x n_prior x n_size x k] */);
/* Waits for the size sweep and copies out weights [W x P x n_size x k] (P = n_prior, 1 for a Jeffreys batch), status
 * [W x P x n_size] - per size: TP_STATUS_NOT_PD when a pivot j < k_s is <= 0 or no larger than k_s 2^-52 times its diagonal
 * element of S1 (of M); TP_STATUS_NONFINITE; TP_STATUS_BAD_DENOM (conjugate): n1 - w1'S1 w1 <= 0 - and aux
 * [W x P x n_size x TP_AUX_STRIDE] (the slots of tp_batch_download's aux: for a Jeffreys batch 0 except slot 4, t'M^-1 t over
 * the prefix); each may be NULL.  Without a size sweep (of either kind) before it: TP_ERR_INVALID. */
int tp_batch_download_size_sweep(tp_batch_t b, double* weights /* [W x P x n_size x k] */,
                                 int32_t* status /* [W x P x n_size] */,
                                 double* aux /* [W x P x n_size x TP_AUX_STRIDE] */);
/* Window sweep: n_len nested window lengths per window - the `rolling_window` axis of a spec grid - from ONE pack, ONE upload
 * and ONE pass over the rows of the longest window.  It rests on the window of length N' < N that ends at a date being the
 * tail of the longer one (ref:159) and on the intraday window not depending on the length at all (ref:299-314); the caller
 * vouches for the universe being the same at every length (batch.pack_windows_lengths checks it).
 * Window w has n_w daily rows (n_rows[w], else n_r) at positions 0 .. n_w-1 as uploaded, oldest first.  Length l uses the last
 * rows[w][l] of them, positions r in [n_w - rows[w][l], n_w).  With x_r the batch's own row (panel - rf_adj), the row of
 * length l is x_r - delta[w][l][r] 1 (delta == NULL: zero) - the per-row risk-free adjustment (ref:48) depends on the mean
 * calendar gap of the length's own labels -, T_l = sum x x' and t_l = sum x over that suffix, and N_l = N[l] replaces
 * tp_params_t.N wherever the definitions of tp_batch_prior_sweep / tp_batch_run read it:
 *   conjugate batch, prior p: C, m, a = n0_wpl m/(m-1) as in tp_batch_prior_sweep, C and w0_wp shared by all lengths;
 *     S1 = a C + T_l ;  q0 = a w0_wp'C w0_wp ;  c = 2 n0_wpl / (g + sqrt(g^2 + 4 n0_wpl q0)),  g = n0_wpl + k + 2
 *     w1 = S1^-1 (c a C w0_wp + t_l) ;  n1 = n0_wpl + N_l ;  weights[w][p][l] = (n1 + k + 2) w1 / (n1 - w1'S1 w1) / gamma
 *   Jeffreys batch: n_prior = 0, n0 = w0 = NULL, the outputs have P = 1: weights[w][0][l] = M^-1 t_l / gamma with
 *     M = T_l - t_l t_l'/N_l (TP_FLAG_CENTER_BY_ROWS: / rows[w][l]; TP_FLAG_NO_CENTER: M = T_l).
 * The batch's own uploaded w0 / n0, its tp_batch_set_rhs and tp_batch_set_shift are not used.
 * TP_ERR_INVALID: a batch that was not uploaded; n_len outside [1, TP_SWEEP_MAX_RHS]; N NULL, not strictly increasing or < 1;
 * rows NULL; a rows[w][l] < 1, > n_w or decreasing in l (ties are allowed: an early date truncates several lengths to the same
 * rows); a non-finite delta at a position some length reads; conjugate: n_prior < 1, n0 or w0 NULL, an n0 that is not finite
 * and > 0, a non-finite w0; Jeffreys: n_prior != 0 or a non-NULL n0 / w0.  TP_ERR_UNSUPPORTED: k > tp_sweep_max_assets() (also:
 * index-layout windows of more than about 10,000 rows).  TP_ERR_HIP: an allocation failed (the message names the byte count).
 * A call refused with TP_ERR_INVALID leaves the results of the last window sweep in place.
 * How it runs: sub-ranges of windows as in tp_batch_prior_sweep ("sweep_chunk_windows"), holding n_len (conjugate: + 1) k x k
 * matrices per window inside 256 MiB.  Per sub-range one Gram pass - one wavefront per window - stores C once, then takes the
 * daily rows through the MFMAs from the newest backwards in n_len segments and stores a snapshot (T_l, t_l) after each: a
 * snapshot is a store, not more flops.  With a delta, one more kernel forms v = sum delta_r x_r, s1 = sum delta_r and
 * s2 = sum delta_r^2 per (window, length); the solve kernel - one workgroup per (window, prior, length) - applies
 * T = G - v 1' - 1 v' + s2 1 1', t = g - s1 1 exactly while it loads the matrix, factorises in LDS and solves.
 * Promises.  A (window, prior, length) result depends on the rows of its own suffix, its delta, its prior, N_l and k.  It does
 * not depend on W, n_prior, the window's position or the sub-ranges: bit for bit.  It depends on the OTHER lengths of the list
 * to rounding only: the list sets where the partial sums of the Gram are cut.  A row older than a length's suffix - NaN, Inf or
 * an outlier - never reaches that length.
 * Device memory: W x P x n_len x (k + 10) doubles of priors and results, W x P x k of w0, W x n_len x k of t, with a delta
 * W x n_len x (n_r + k + 2) more - the copy of delta and its sums; 10,000 dates x 4 lengths x 499 rows: 160 MB, outside the
 * 256 MiB rule -, and the sub-range's matrices; kept until tp_batch_destroy.  Streams, the entry
 * drain, timing (kernel_ms covers every launch; one step of tp_region_steps), the gather hand-over and what the call leaves
 * alone are as for tp_batch_size_sweep; it has result buffers of its own: every other download returns what it returned
 * before. */
int tp_batch_window_sweep(tp_batch_t b, int32_t n_len, const int32_t* N /* [n_len] */,
                          const int32_t* rows /* [W x n_len] */,
                          const double* delta /* [W x n_len x n_r] or NULL */,
                          int32_t n_prior, const double* n0 /* [W x n_prior x n_len] */,
                          const double* w0 /* [W x n_prior x k] */);
/* tp_batch_window_sweep above tp_sweep_max_assets(), on the large-k tiled pipeline: the same definition, arguments,
 * validation and result buffers (tp_batch_download_window_sweep serves both calls; a call refused with TP_ERR_INVALID leaves
 * the results of the last window sweep of either kind in place).
 * TP_ERR_UNSUPPORTED: k <= tp_sweep_max_assets() (tp_batch_window_sweep serves those).  No limit on the rows of an index-layout
 * window: the rows are not staged.
 * How it runs: sub-ranges of windows under the same rule ("sweep_chunk_windows", n_len (conjugate: + 1) k x k matrices per
 * window, at least one window) inside 4 GiB, not 256 MiB: the entries are factorised in groups of one length, and the
 * sub-range decides how full those launches run.  Per sub-range, conjugate: the batch's own tiled Gram stage runs ONCE per window
 * over the intraday rows, steered by its arguments as in tp_batch_prior_sweep_tiled, so C is RAW-MOMENT centred (exact to
 * rounding for returns, it loses digits under a large common offset of the intraday panel) and never comes from the shared
 * intraday sums.  Then a segmented Gram - one wavefront per (window, 64 x 64 super-tile), 16 tiles in registers, cleared once -
 * takes the daily rows through the MFMAs from the newest backwards in n_len segments and stores its part of (T_l, t_l) after
 * each: max rows[w][l] rows pass the MFMAs, not their sum, and never the shared daily sums.  With a delta the delta kernel of
 * tp_batch_window_sweep forms v, s1 and s2.  C w0_wp and w0_wp'C w0_wp are formed once per (window, prior).  The
 * (window, prior, length) entries then go through the batch's RUN workspace (borrowed as by tp_batch_prior_sweep_tiled, and
 * grown to hold up to the sub-range's window x prior pairs where the arena budget allows) in groups of ONE length: a fill kernel
 * applies T = G - v 1' - 1 v' + s2 1 1', t = g - s1 1 from left to right (a zero delta gives the bits of delta == NULL), the
 * tiled factorisation and solve of tp_batch_run run with N = N[l], and the results are copied to their slots.
 * Statuses are those of tp_batch_run on the large-k path: TP_STATUS_NOT_PD is a pivot that is not > 0 - there is no relative
 * floor, so a Jeffreys length of fewer rows than columns gets whatever tp_batch_run gives a batch of that suffix -,
 * TP_STATUS_NONFINITE and (conjugate) TP_STATUS_BAD_DENOM come from the solve.  Aux as in tp_batch_download_window_sweep.
 * Promises.  A (window, prior, length) result depends on the rows of its own suffix, its delta, its prior, N_l and k.  It does
 * not depend on W, n_prior, the window's position, the sub-ranges or the arena's size ("tiled_arena_mib"): bit for bit.  It
 * depends on the OTHER lengths of the list to rounding only.  A row older than a length's suffix - NaN, Inf or an outlier -
 * never reaches that length: its snapshot has left the registers before that row is loaded.
 * Device memory: that of tp_batch_window_sweep plus, conjugate, (k + 1) doubles per (window, prior) of a sub-range, k + 9
 * doubles per entry of one group, and the run workspace - which stays grown afterwards, as after tp_batch_prior_sweep_tiled;
 * kept until tp_batch_destroy.  Streams, the entry drain, timing (kernel_ms covers every launch; one step of tp_region_steps),
 * the gather hand-over and what the call leaves alone are as for tp_batch_prior_sweep_tiled; every other download returns what
 * it returned before. */
int tp_batch_window_sweep_tiled(tp_batch_t b, int32_t n_len, const int32_t* N /* [n_len] */,
                                const int32_t* rows /* [W x n_len] */,
                                const double* delta /* [W x n_len x n_r] or NULL */,
                                int32_t n_prior, const double* n0 /* [W x n_prior x n_len] */,
                                const double* w0 /* [W x n_prior x k] */);
/* Waits for the window sweep and copies out weights [W x P x n_len x k] (P = n_prior, 1 for a Jeffreys batch), status
 * [W x P x n_len] (TP_STATUS_OK; TP_STATUS_NOT_PD: a pivot <= 0 or no larger than k 2^-52 times its diagonal element, e.g. a
 * Jeffreys length of fewer rows than columns; TP_STATUS_NONFINITE; TP_STATUS_BAD_DENOM (conjugate): n1 - w1'S1 w1 <= 0) and aux
 * [W x P x n_len x TP_AUX_STRIDE] (the slots of tp_batch_download's aux: for a Jeffreys batch 0 except slot 4, t'M^-1 t); each
 * may be NULL.  After tp_batch_window_sweep_tiled the statuses are those of the large-k path (no relative pivot floor).  Without
 * a window sweep (of either kind) before it: TP_ERR_INVALID. */
int tp_batch_download_window_sweep(tp_batch_t b, double* weights /* [W x P x n_len x k] */,
                                   int32_t* status /* [W x P x n_len] */,
                                   double* aux /* [W x P x n_len x TP_AUX_STRIDE] */);
/* Grid sweep: n_size nested universes x n_len nested window lengths per window - the `size` and `rolling_window` axes of a spec
 * grid crossed (ref: portfolio_specs.py:71-72) - from ONE pack, ONE upload, ONE pass over the rows of the longest window at the
 * largest size and ONE factorisation per (window, prior, length).  It rests on both nestings at once: the columns are ordered so
 * that the smaller universe is a prefix of the larger one (tp_batch_size_sweep) and the shorter window is the tail of the longer
 * one (tp_batch_window_sweep); the caller vouches for both at every (size, length) (batch.pack_windows_grid checks them).
 * Entry (w, p, l, s), with k_s = sizes[s], the rows, delta, T_l, t_l and N_l = N[l] of tp_batch_window_sweep:
 *   conjugate batch: what tp_batch_run returns for a batch of size k_s over the prefix columns and the last rows[w][l] rows,
 *     minus delta[w][l], with (w0_wps, n0_wpl) uploaded and N = N[l] (not bit for bit: the factorisation differs):
 *     S1 = (a C + T_l)[:k_s,:k_s], a = n0_wpl m/(m-1) ;  v = C[:k_s,:k_s] w0_wps[:k_s] ;  q0 = a w0_wps'v
 *     c = 2 n0_wpl / (g + sqrt(g^2 + 4 n0_wpl q0)),  g = n0_wpl + k_s + 2 ;  w1 = S1^-1 (c a v + t_l[:k_s]) ;  n1 = n0_wpl + N_l
 *     weights[w][p][l][s][:k_s] = (n1 + k_s + 2) w1 / (n1 - w1'S1 w1) / gamma ,   weights[w][p][l][s][k_s:] = 0
 *   Jeffreys batch: n_prior = 0, n0 = w0 = NULL, the outputs have P = 1: weights[w][0][l][s][:k_s] = M[:k_s,:k_s]^-1 t_l[:k_s] / gamma
 *     with M = T_l - t_l t_l'/N_l (TP_FLAG_CENTER_BY_ROWS: / rows[w][l]; TP_FLAG_NO_CENTER: M = T_l) - the size sweep's definition
 *     on length l's rows.
 * Only the first k_s entries of a w0 vector are read.  The batch's own uploaded w0 / n0, its tp_batch_set_rhs and
 * tp_batch_set_shift are not used.
 * TP_ERR_INVALID: a batch that was not uploaded; n_size or n_len outside [1, TP_SWEEP_MAX_RHS]; sizes NULL or not strictly
 * increasing within [1, k]; N NULL, not strictly increasing or < 1; rows NULL; a rows[w][l] < 1, > n_w or decreasing in l (ties
 * are allowed); a non-finite delta at a position some length reads; conjugate: n_prior < 1, n0 or w0 NULL, an n0 that is not
 * finite and > 0, a non-finite w0 inside a prefix; Jeffreys: n_prior != 0 or a non-NULL n0 / w0.  All of them are found before
 * any device work, and a call refused with TP_ERR_INVALID leaves the results of the last grid sweep in place.
 * TP_ERR_UNSUPPORTED: k > tp_sweep_max_assets() (also: index-layout windows of more than about 10,000 rows).  TP_ERR_HIP: an
 * allocation failed (the message names the byte count).
 * How it runs: sub-ranges of windows as in tp_batch_window_sweep ("sweep_chunk_windows", n_len (conjugate: + 1) k x k matrices
 * per window inside 256 MiB).  Per sub-range the Gram pass and - with a delta - the delta kernel of tp_batch_window_sweep run
 * as they are; then one workgroup per (window, prior, length) loads the matrix with the rank-two correction applied from left
 * to right, parks one right-hand side per size behind it (conjugate: the truncated products C[:k_s,:k_s] w0_wps come from the
 * same pass over C, masked, never multiplied by zero), factorises ONCE in LDS at k and back-substitutes every size over its own
 * prefix: n_len x n_prior factorisations per window where one window sweep per size takes n_size times as many.
 * Promises.  An entry depends on the rows of its own suffix, its delta, its prior, N_l, k_s and k.  It does not depend on the
 * OTHER sizes of the list, on W, n_prior, the window's position or the sub-ranges: bit for bit.  It depends on the other
 * lengths to rounding only (the list sets where the partial sums of the Gram are cut).  An all-zero delta gives the bits of
 * delta == NULL.  A column at or beyond k_s - a duplicate, a zero column, a NaN - does not reach size s; a row older than a
 * length's suffix never reaches that length.
 * Device memory: W x P x n_len x n_size x (k + 9) doubles of results, W x P x n_size x k of w0, W x P x n_len of n0,
 * W x n_len x k of t, with a delta W x n_len x (n_r + k + 2) more, and the sub-range's matrices - buffers of its own, kept until
 * tp_batch_destroy: every other download, tp_batch_download_window_sweep and _size_sweep included, returns what it returned
 * before.  Streams, the entry drain, timing (kernel_ms covers every launch; one step of tp_region_steps) and the gather
 * hand-over are as for tp_batch_window_sweep. */
int tp_batch_grid_sweep(tp_batch_t b, int32_t n_size, const int32_t* sizes /* [n_size] */,
                        int32_t n_len, const int32_t* N /* [n_len] */, const int32_t* rows /* [W x n_len] */,
                        const double* delta /* [W x n_len x n_r] or NULL */,
                        int32_t n_prior, const double* n0 /* [W x n_prior x n_len] */,
                        const double* w0 /* [W x n_prior x n_size x k] */);
/* tp_batch_grid_sweep above tp_sweep_max_assets(), on the large-k tiled pipeline: the same definition of entry (w, p, l, s),
 * arguments, validation and result buffers (tp_batch_download_grid_sweep serves both calls; a call refused with TP_ERR_INVALID
 * leaves the results of the last grid sweep of either kind in place).  Single sizes may be anything in [1, k], sizes
 * <= tp_sweep_max_assets() included: they ride along as prefixes of the same entries.
 * TP_ERR_UNSUPPORTED: k <= tp_sweep_max_assets() (tp_batch_grid_sweep serves those); k + n_size > tp_max_assets() + 1 (the
 * right-hand sides of the sizes travel in columns k .. k + n_size - 1 of an arena of side 64 ceil((k + n_size)/64) <= 2048).  No
 * limit on the rows of an index-layout window: the rows are not staged.
 * How it runs: sub-ranges of windows under the rule and the 4 GiB budget of tp_batch_window_sweep_tiled ("sweep_chunk_windows",
 * n_len (conjugate: + 1) k x k matrices per window, at least one window).  Per sub-range, conjugate: the batch's own tiled Gram
 * stage runs ONCE per window over the intraday rows, steered by its arguments as in tp_batch_prior_sweep_tiled, so C is
 * RAW-MOMENT centred (exact to rounding for returns, it loses digits under a large common offset of the intraday panel) and
 * never comes from the shared intraday sums; it goes through the batch's run workspace, which is not grown.  The segmented Gram
 * of tp_batch_window_sweep_tiled stores (T_l, t_l) per length at the batch's k from ONE pass over the daily rows, and with a
 * delta the delta kernel forms v, s1 and s2.  One kernel per (window, prior) forms the n_size truncated products
 * v_s = C[:k_s,:k_s] w0_wps[:k_s] and w0_wps'v_s in one pass over the rows of C - terms at or beyond k_s selected out, never
 * multiplied by zero; they depend on neither the length nor n0.  An ENTRY is a (window, prior, length); the entries of a sub-range
 * go through the tiled solve sweep's workspace at R = n_size (shared with tp_batch_solve_sweep_tiled and
 * tp_batch_size_sweep_tiled, whose downloads are left alone) in groups of its capacity, ALL lengths together: a fill kernel writes
 * a C + (G_l - v 1' - 1 v' + s2 1 1') - the correction from left to right - or the Jeffreys matrix inside k x k and the
 * right-hand side of size s into rows < k_s of column k + s, exact zeros elsewhere; the block steps of the tiled factorisation
 * factorise ONCE at k and forward-substitute the columns; the solve kernel reads N_l and n0_wpl per entry, back-substitutes every
 * size over its own prefix and writes weights, statuses and aux rows straight to their slots.
 * Statuses per size are those of tp_batch_download_grid_sweep (the relative pivot floor over the prefix, from the diagonal the
 * fill stored); the entry's own not-positive-definite flag decides no size.
 * Promises.  Bit for bit: an entry does not depend on W, n_prior, the window's or the prior's slot, the sub-ranges or the arena's
 * size ("tiled_arena_mib"); an all-zero delta gives the bits of delta == NULL.  To rounding only: an entry depends on the OTHER
 * lengths of the list (the list sets where the partial sums of the Gram are cut) and on the other SIZES (n_size sets the arena's
 * side, as in tp_batch_size_sweep_tiled).  A row older than a length's suffix never reaches that length.  Columns at or beyond a
 * prefix: a finite degenerate column j (a duplicate, a zero column) leaves every k_s <= j intact and flags the sizes > j; a
 * NON-FINITE column j leaves k_s <= 64 floor(j/64) intact, the sizes in (64 floor(j/64), j] may come back flagged - the block
 * steps multiply whole 64-row blocks with MFMAs, where a structural zero times a NaN is a NaN - and the sizes > j are flagged.
 * No size is TP_STATUS_OK with numbers that are not its own.
 * Device memory: that of tp_batch_grid_sweep plus, conjugate, n_size (k + 1) doubles per (window, prior) of a sub-range and, per
 * entry of the sweep's workspace, KP^2 + 4096 ceil(k/64) + k doubles - as many entries as the arena budget allows
 * ("tiled_arena_gib" / "tiled_arena_mib"); kept until tp_batch_destroy.  Streams, the entry drain, timing (kernel_ms covers every
 * launch; one step of tp_region_steps), the gather hand-over and what the call leaves alone are as for tp_batch_grid_sweep. */
int tp_batch_grid_sweep_tiled(tp_batch_t b, int32_t n_size, const int32_t* sizes /* [n_size] */,
                              int32_t n_len, const int32_t* N /* [n_len] */, const int32_t* rows /* [W x n_len] */,
                              const double* delta /* [W x n_len x n_r] or NULL */,
                              int32_t n_prior, const double* n0 /* [W x n_prior x n_len] */,
                              const double* w0 /* [W x n_prior x n_size x k] */);
/* Waits for the grid sweep and copies out weights [W x P x n_len x n_size x k] (P = n_prior, 1 for a Jeffreys batch), status
 * [W x P x n_len x n_size] - per entry: TP_STATUS_NOT_PD when a pivot j < k_s is <= 0 or no larger than k_s 2^-52 times its
 * diagonal element of S1 (of M), e.g. a Jeffreys length of fewer rows than k_s; TP_STATUS_NONFINITE; TP_STATUS_BAD_DENOM
 * (conjugate): n1 - w1'S1 w1 <= 0 - and aux [W x P x n_len x n_size x TP_AUX_STRIDE] (the slots of tp_batch_download's aux: for
 * a Jeffreys batch 0 except slot 4, t_l'M^-1 t_l over the prefix); each may be NULL.  Without a grid sweep (of either kind)
 * before it: TP_ERR_INVALID. */
int tp_batch_download_grid_sweep(tp_batch_t b, double* weights /* [W x P x n_len x n_size x k] */,
                                 int32_t* status /* [W x P x n_len x n_size] */,
                                 double* aux /* [W x P x n_len x n_size x TP_AUX_STRIDE] */);
int tp_batch_download(tp_batch_t b, double* weights /* [W x k] */, int32_t* status /* [W] */,
                      double* aux /* optional [W x TP_AUX_STRIDE] */); /* waits for the stream, D2H */
int tp_batch_download_S1(tp_batch_t b, int64_t w, double* S1 /* [k x k] */); /* posterior scale matrix
                      S1 (ref:358) / Jeffreys J (ref:600) of window w, recomputed by a debug launch */
/* Read back one window's k x k matrix (symmetric, full storage) and its k-vector, recomputed by a
 * one-window launch; `rhs` may be NULL.  The reference's same-named helper functions bind these.
 * TP_MATRIX_PRIOR centres the intraday rows first (two passes, like DataFrame.cov, ref:317), so every entry of S0
 * has the relative accuracy of the reference's own; a run forms the same matrix in one pass, equal to rounding in
 * the norm.  Register-tile path only (k <= 239): TP_ERR_UNSUPPORTED above. */
#define TP_MATRIX_PRIOR 1      /* S0 (ref:285-333)            and c S0 w0                     */
#define TP_MATRIX_GRAM 2       /* T  (ref:163-204)            and t (ref:206-245)             */
#define TP_MATRIX_POSTERIOR 3  /* S1 (ref:358) / J (ref:600)  and c S0 w0 + t (ref:489) / t   */
int tp_batch_download_matrix(tp_batch_t b, int64_t w, int what, double* M /* [k x k] */, double* rhs /* [k] */);
/* Diagnostic builds only (make TP_STAMP=1; otherwise TP_ERR_UNSUPPORTED): run the batch once and return
 * 40 values per window: eight shader-clock stamps at the kernel's phase boundaries, then per wave (4)
 * the summed cycles of the four segments of the daily Gram loop (loads | MFMA | LDS write | barrier),
 * then for waves 0 and 1 those of a factorisation block step (hand-over | elimination | TRSM | trailing). */
int tp_batch_debug_stamps(tp_batch_t b, int64_t* stamps /* [W x 40] */);
int tp_batch_destroy(tp_batch_t b);

/* One-shot convenience: upload + run + download.  Replaces
 * calculate_conjugate_hf_mcm_portfolio (ref:819) / calculate_jeffreys_portfolio (ref:838) over W dates. */
int tp_posterior_batch(tp_handle_t h, const tp_params_t* p, int64_t W, const tp_inputs_t* in,
                       double* weights, int32_t* status, double* aux);

/* Backtest replay: the daily loop of ref:1127-1219 - mark to market, weight drift, rebalance, turnover (ref:1054-1075), weight
 * metrics and the distance to the value-weighted portfolio (ref:1077-1104) - for MANY portfolios whose weights at every
 * rebalancing date are already in hand (a sweep's download, a spec grid), one wavefront per portfolio in one launch.  Replaces
 * the loop over dates of backtest_portfolio (ref:1232) around Portfolio.update_portfolio, per spec.
 *
 * tp_replay_merge_maps needs no device.  For a universe table cols [R x k] (row j at cols + j * stride; entries are ticker
 * indices in [0, K), no ticker twice in a row) it fills, both [R x k] dense:
 *     prev_slot[j][i] = the slot ticker cols[j][i] held at date j-1, or -1 (row 0: all -1)
 *     next_slot[j][i] = the slot ticker cols[j][i] holds at date j+1, or -1 (row R-1: all -1)
 * so that the outer merge of the turnover needs no table of K entries on the device.  TP_ERR_INVALID: an index outside [0, K),
 * a ticker twice in one row, R < 1, k < 1, K < 1, stride < 0, a NULL pointer (tp_last_error(NULL) has the message). */
int tp_replay_merge_maps(const int32_t* cols, int64_t R, int32_t k, int64_t stride, int32_t K,
                         int32_t* prev_slot /* [R x k] */, int32_t* next_slot /* [R x k] */);
/* One call for all portfolios that share trading days and a rebalancing schedule; every pointer is a HOST pointer.
 * Shared: S [D x ld] simple returns of trading day d (row 0 is not read; NaN allowed), of which the first K columns are tickers;
 * rf_daily [D]; reb_day [R] the trading-day index of every rebalancing date, strictly increasing, reb_day[0] == 0, all < D.
 * Portfolio p < P holds k[p] assets; at rebalancing date j its weights are weights[w_off[p] + j w_stride[p] + i], its tickers
 * cols[u_off[p] + j u_stride[p] + i] and their market caps caps[u_off[p] + j u_stride[p] + i], i < k[p] - offsets and strides in
 * elements, so that a sweep's download [W x P x n_len x n_size x k] is replayed where it lies and the specs of one family
 * share one universe table.  weights_len / universe_len: elements of the flat buffers (cols and caps have one shape).
 * Per trading day d >= 1, in the operations and order of ref:1131-1164 with the NaN-skipping sums pandas uses:
 *     r_i = S[d][col_i] ;  cash = 1 - nansum(w) ;  returns[p][d] = nansum(r w) + cash rf_daily[d]
 *     drifted = w (1 + r) ;  total = nansum(drifted) + cash (1 + rf_daily[d]) ;  w = drifted / total
 *     |(sum(w) + cash (1 + rf_daily[d]) / total) - 1| > 1e-5 (plain sum: a NaN never trips it): status[p] = TP_REPLAY_SUM_CHECK,
 *     bad_day[p] = d, the portfolio's outputs from that day and rebalancing date on are NaN and its loop ends (ref:1160-1162)
 * and per rebalancing date j, after the day's mark to market: metrics[p][j] = max_long, max_short, avg_long, avg_short (NaN for
 * an empty side; the first two are selections, bit-equal to the input weight) and nanmean |w scaling[p] - caps / nansum(caps)|;
 * for j > 0 turnover[p][j] = (sum over the union of |before - after|, a missing or NaN entry as 0, + |nansum(before) -
 * nansum(after)|) / 2 and returns[p][reb_day[j]] -= cost[p] / 10000 * turnover[p][j] (ref:1212).
 * Every sum is a lane-local partial sum in slot order and a fixed 64-lane tree: a portfolio's results are the same bit for bit
 * from run to run, alone or among others, packed densely or in place.  Against the host's summation order they agree to
 * rounding.
 * TP_ERR_INVALID: D, R, P, ld, K out of range, a NULL array, reb_day[0] != 0 or not strictly increasing below D, k[p] < 1, an
 * offset or stride that is negative or runs past its buffer (checked without overflow), a column index outside [0, K), a ticker
 * twice in one row.  TP_ERR_UNSUPPORTED: k[p] > tp_max_assets().  TP_ERR_HIP: an allocation failed (the message names the byte
 * count).  The merge maps are built inside the call, once per distinct (u_off, u_stride, k).
 * The call waits for whatever was queued on the handle's stream, copies every input to the device (no host pointer is kept),
 * and queues one launch per slots-per-lane class (k <= 64, 128, 256, ...) without waiting for it.  kernel_ms of tp_last_timing
 * covers the launches (one HIP-event pair; one step of tp_region_steps); tp_last_launch keeps describing tp_batch_run.  The
 * buffers belong to the handle and are kept until tp_destroy; batches and their results are left alone. */
#define TP_REPLAY_SUM_CHECK 1 /* status[p]: "Weights do not sum to 1." (ref:1160-1162) on day bad_day[p] */
int tp_replay_run(tp_handle_t h, int64_t D, int32_t ld, const double* S /* [D x ld] */, const double* rf_daily /* [D] */,
                  int64_t R, const int32_t* reb_day /* [R] */, int32_t K,
                  int64_t P, const int32_t* k /* [P] */, const double* scaling /* [P] */, const double* cost /* [P] */,
                  const int64_t* w_off /* [P] */, const int64_t* w_stride /* [P] */,
                  const int64_t* u_off /* [P] */, const int64_t* u_stride /* [P] */,
                  const double* weights, int64_t weights_len, const int32_t* cols, const double* caps, int64_t universe_len);
/* tp_replay_run with the weights read where a batch's results already lie on the device: no download, no repacking, no upload
 * of the weights - only the small inputs go up and tp_replay_download brings the results down.  The daily loop, the merge maps,
 * the universe tables (cols, caps: HOST pointers, uploaded), the launch classes, the outputs on the handle of `b` and every
 * argument tp_replay_run also has are tp_replay_run's.  What differs is where a weight row comes from.  `source` names the
 * results - those of the batch's LAST call of that kind (TP_REPLAY_SRC_RUN: the pair the last tp_batch_run wrote) -, w_off /
 * w_stride index its weights and s_off / s_stride its statuses, in elements, as the matching download lays them out.  For
 * portfolio p, rebalancing date j and slot i < k[p]:
 *   patched - (p, j) is (patch_port[q], patch_date[q]) for some q -: the weight is patch_weights[q patch_ld + i] as it is: no
 *     scale, no status consulted.  Patches are HOST arrays, sorted by (patch_port, patch_date), strictly increasing; a portfolio
 *     may have all R dates patched and then never touches the source;
 *   otherwise: the weight is fl(w_scale[p] * src[w_off[p] + j w_stride[p] + i]) - ONE rounding (what the host forms as
 *     1.0 / gamma * w when a batch ran with gamma = 1); w_scale == NULL means ones, and a scale of exactly 1.0 leaves the bits
 *     alone.  The row's status is srcstatus[s_off[p] + j s_stride[p]]: when it is not TP_STATUS_OK, status[p] =
 *     TP_REPLAY_BAD_WEIGHTS, bad_day[p] = reb_day[j], the portfolio's returns from that day on and its turnover and metrics from
 *     date j on are NaN and its loop ends - the exit of the sum check, which wins when it trips on the same day (it comes first
 *     in the day).  A row that is flagged may hold anything, NaN included: it is ordinary data.
 * The patch lookup costs nothing per day: a wave keeps a cursor into its portfolio's sorted patches and compares once per
 * rebalancing date.
 * TP_ERR_INVALID, all checked before anything is uploaded or launched (a refused call leaves the last replay's results in
 * place): everything tp_replay_run refuses; an unknown source; a source the batch has no results for (no run or sweep of that
 * kind yet); a w_off / w_stride that runs past the source's weights or an s_off / s_stride that runs past its statuses (R rows
 * of k[p], R rows of 1: patched dates included; without overflow); n_patch < 0; unsorted or repeated patches; a patch_port
 * outside [0, P); a patch_date outside [0, R); patch_ld smaller than the k of a patched portfolio; a NULL array that is needed
 * (w_scale may be NULL; the patch arrays when n_patch == 0).  TP_ERR_UNSUPPORTED, TP_ERR_HIP: as tp_replay_run.
 * Streams: the call waits on entry for whatever is queued on the handle's stream - this is where the sweep finishes -, uploads
 * the inputs, queues the launches and does not wait for them; a later run or sweep of the batch is ordered behind them by the
 * stream, tp_batch_destroy drains it.  The call writes nothing into the batch: every tp_batch_download* returns afterwards the
 * bytes it returned before.  kernel_ms, tp_region_steps and tp_last_launch: as tp_replay_run. */
#define TP_REPLAY_SRC_RUN          0  /* tp_batch_run:                 weights [W x k],              status [W]            */
#define TP_REPLAY_SRC_PRIOR_SWEEP  1  /* tp_batch_prior_sweep[_tiled]:  [W x P x k],                  [W x P]               */
#define TP_REPLAY_SRC_SIZE_SWEEP   2  /* tp_batch_size_sweep[_tiled]:   [W x P x S x k],              [W x P x S]           */
#define TP_REPLAY_SRC_WINDOW_SWEEP 3  /* tp_batch_window_sweep[_tiled]: [W x P x L x k],              [W x P x L]           */
#define TP_REPLAY_SRC_GRID_SWEEP   4  /* tp_batch_grid_sweep[_tiled]:   [W x P x L x S x k],          [W x P x L x S]       */
#define TP_REPLAY_SRC_SWEEP_FINISH 5  /* tp_batch_sweep_finish:         weights [W x k],              status [W]            */
#define TP_REPLAY_SRC_SPECTRAL     6  /* tp_batch_spectral_greyserman:  weights [W x k],              status [W]            */
#define TP_REPLAY_BAD_WEIGHTS 2       /* status[p]: a weight row was read whose source status was not TP_STATUS_OK */
int tp_replay_run_batch(tp_batch_t b, int source,
                        int64_t D, int32_t ld, const double* S, const double* rf_daily,
                        int64_t R, const int32_t* reb_day, int32_t K,
                        int64_t P, const int32_t* k, const double* scaling, const double* cost,
                        const double* w_scale /* [P] or NULL: ones */,
                        const int64_t* w_off, const int64_t* w_stride,   /* into the SOURCE's weights on the device */
                        const int64_t* s_off, const int64_t* s_stride,   /* into the SOURCE's statuses on the device */
                        const int64_t* u_off, const int64_t* u_stride,
                        const int32_t* cols, const double* caps, int64_t universe_len,
                        int64_t n_patch, const int64_t* patch_port /* [n_patch] */, const int32_t* patch_date /* [n_patch] */,
                        const double* patch_weights /* [n_patch x patch_ld] */, int32_t patch_ld);
/* Waits for the replay and copies out returns [P x D] (returns[p][0] is NaN), turnover [P x R] (turnover[p][0] is NaN), metrics
 * [P x R x 5], status [P] (0, TP_REPLAY_SUM_CHECK or - tp_replay_run_batch - TP_REPLAY_BAD_WEIGHTS) and bad_day [P] (-1 without
 * a status); each may be NULL.  Without a tp_replay_run or tp_replay_run_batch before it: TP_ERR_INVALID. */
int tp_replay_download(tp_handle_t h, double* returns, double* turnover, double* metrics, int32_t* status, int32_t* bad_day);

/* Performance summary of the last replay on the handle (tp_replay_run or tp_replay_run_batch) over a grid of C trading costs:
 * the statistics the evaluation of ref:464-701 (performance_metrics) takes from a strategy's daily returns, reduced on the
 * device to one record of TP_SUMMARY_STATS doubles per (portfolio, cost), one wavefront each; only the records come down.  A
 * cost never touches the holdings - it enters a replay only through ref:1212 - so ONE replay at cost 0 carries every cost.
 * All operations in double, one rounding each.  For portfolio p, cost c and n = D - 1 (day 0 is never read), d = 1 .. D-1:
 *   net return x_d = returns[p][d] as stored; on a day d = reb_day[j] with j >= 1 it is
 *     fl(returns[p][d] - fl(fl(cost_bp[c] / 10000) turnover[p][j])) - with the replay run at cost 0, bit for bit the returns of a
 *     replay run at cost c.  On every other day the stored value is selected: no turnover reaches it;
 *   excess return e_d = fl(x_d - rf_excess[d]) (ref:712-713; the caller forms rf_excess);
 *   adjust_returns (ref:46-72), applied to x and to e separately (ref:484, 488): with W_i = prod_{d <= i} (1 + a_d), at the first i
 *     with W_i - 1 < -1: a_i = -1 if i is day 1, else a_i = 0.000001 / (W_{i-1} - 1) - 1 (as the reference wrote it, a division
 *     by zero included); every later day is 0.  The adjusted series are a (from x) and b (from e);
 *   insolvency (ref:27-33): the first d with W_d - 1 < -0.99 on a.
 * The record, in this order:
 *    0 N_OBS n;  1 ADJ_DAY the trading day adjust_returns changed in a, -1: none;  2 INSOLVENT_DAY, -1: none;
 *    3 COMP W_{D-1} - 1 of a;  4 MEAN, 5 STD of a (two passes, ddof = 1, NaN for n < 2);
 *    6 MAX_DD min_d W_d / max_{d' <= d} W_d' - 1, the running peak starting at W_1 (NaN when that peak is 0: day 1 was
 *      adjusted and every quotient is 0 / 0);  7 BEST, 8 WORST of a (selections);
 *    9 SUM_WIN, 10 N_WIN over a > 0;  11 SUM_LOSS, 12 N_LOSS over a < 0;
 *   13 N_PRE, 14 MEAN_PRE, 15 STD_PRE, 16 WORST_PRE over the days d < INSOLVENT_DAY (ref:644, 660, 670; all days without one;
 *      NaN where N_PRE is too small);  17 SUM_NONZERO, 18 N_NONZERO over |a| > 1e-7 (ref:612);
 *   19 ADJ_DAY_E as ADJ_DAY, for b;  20 MEAN_E, 21 STD_E (ddof = 1) of b;  22-24 M2_E, M3_E, M4_E = sum (b - MEAN_E)^k / n, the
 *      biased central moments;  25 DOWNSIDE_E sum_{b < 0} b^2 / n;
 *   26 TURNOVER_SUM, 27 TURNOVER_N over j = 1 .. R-1 with reb_day[j] <= INSOLVENT_DAY (ref:696; all j without one);
 *   28-31 reserved, 0.0.
 * status[p][c]: TP_SUMMARY_OK; TP_SUMMARY_NO_REPLAY - the replay's status[p] is set: fields 0-27 are NaN; TP_SUMMARY_NONFINITE - a
 * or b holds a NaN or an infinity: fields 0, 1, 2 and 19 are kept, the other fields below 28 are NaN (no NaN-skipping).
 * Days go through in tiles of 64, the products are a six-step scan across the wave times the carry of the tile before, every
 * sum is a lane-local partial in tile order and the replay's fixed 64-lane tree: a record is the same bit for bit from run to
 * run, for a portfolio alone or among others, for a cost alone or among others.  Against a sequential host loop it agrees to
 * rounding.
 * TP_ERR_INVALID, all checked before anything is waited for, uploaded or launched (a refused call leaves the last replay's and
 * the last summary's results in place): no replay before it; a replay of D < 2 days; C < 1 or C > TP_SUMMARY_MAX_COSTS; a NULL
 * array; a cost that is not finite (rf_excess may hold NaN: TP_SUMMARY_NONFINITE).
 * The call waits on entry for whatever is queued on the handle's stream - the replay ends here -, uploads cost_bp and
 * rf_excess (HOST pointers, not kept) and queues one launch without waiting for it.  The replay's results are not written:
 * tp_replay_download returns the same bytes before and after.  kernel_ms, tp_region_steps and tp_last_launch: as tp_replay_run. */
#define TP_SUMMARY_STATS 32
#define TP_SUMMARY_MAX_COSTS 64
#define TP_SUMMARY_OK 0
#define TP_SUMMARY_NO_REPLAY 1
#define TP_SUMMARY_NONFINITE 2
int tp_replay_summary(tp_handle_t h, int32_t C, const double* cost_bp /* [C] */, const double* rf_excess /* [D] */);
/* Waits for the summary and copies out stats [P x C x TP_SUMMARY_STATS] and status [P x C]; each may be NULL.  TP_ERR_INVALID
 * without a tp_replay_summary before it, or when a newer replay has replaced the one it read. */
int tp_replay_download_summary(tp_handle_t h, double* stats, int32_t* status);

int tp_synchronize(tp_handle_t h);
/* Timings of the most recent call of each kind on this handle, in milliseconds (HIP events on the
 * handle's stream): posterior kernel, H2D upload, D2H download, RCCL gather. */
int tp_last_timing(tp_handle_t h, double* kernel_ms, double* h2d_ms, double* d2h_ms, double* gather_ms);
/* HIP-event bracket on the handle's stream around any sequence of tp_batch_run calls (bench.py's
 * timed region): begin records an event, end records another, waits for it and returns the span. */
int tp_region_begin(tp_handle_t h);
int tp_region_end(tp_handle_t h, double* ms);
/* Kernel time of every tp_batch_run inside the last region (each launch is bracketed by its own pair of HIP events on
 * the kernel stream; nothing waits between the steps; at most 512 steps are kept): bench.py's per-step median.
 * step_ms may be NULL (n_steps only). */
int tp_region_steps(tp_handle_t h, double* step_ms, int capacity, int* n_steps);
/* Launch geometry of the most recent tp_batch_run: grid size, threads per workgroup, LDS bytes,
 * 16-column tile count per side. */
int tp_last_launch(tp_handle_t h, int* grid, int* block, int* lds_bytes, int* ntile);

/* Multi-GPU: one process (handle) per GPU; windows are sharded by the caller; the only data-path
 * collective is one gather of the [W_local x k] weights (and statuses) to `root` over RCCL/xGMI.
 * The 128-byte id comes from rank 0 (tp_comm_unique_id) and is distributed by the launcher. */
#define TP_UNIQUE_ID_BYTES 128
int tp_comm_unique_id(void* id /* [TP_UNIQUE_ID_BYTES] */);
int tp_comm_init(tp_handle_t h, const void* id, int rank, int world);
int tp_comm_destroy(tp_handle_t h);
int tp_comm_count(tp_handle_t h, int* ranks);              /* ncclCommCount of the handle's communicator */
/* Single-process form (main.py is ONE process, src/main.py:26): one communicator over the n handles of this
 * process, rank i = handles[i], one handle per GPU (ncclCommInitAll; no id exchange, no launcher).
 * tp_group_gather is tp_batch_gather for it: batches[i] on rank i, all with the same W (pad the last shard),
 * every rank's gather issued in one group by the calling thread; waits; optional host copy-out on the root. */
int tp_comm_init_all(tp_handle_t* handles, int n);
int tp_group_gather(tp_batch_t* batches, int n, int root, double* weights_all /* [n x W x k] or NULL */,
                    int32_t* status_all /* [n x W] or NULL */);
/* Every rank calls it with the same W_local.  The gathered [world x W x k] weights and [world x W]
 * statuses stay in root's HBM; weights_all / status_all are optional HOST buffers on root (NULL: no
 * copy-out, fetch later with tp_batch_download_gathered). */
int tp_batch_gather(tp_batch_t b, int root, double* weights_all, int32_t* status_all);
/* The same gather without waiting for it, on a second, high-priority stream: from its first use the batch
 * keeps TWO result buffers and tp_batch_run alternates between them, so the gather of step i reads one while
 * the kernel of step i+1 writes the other (a rebalancing schedule that streams batches); no copy is made.
 * The call only REQUESTS the gather: it is put on its stream inside the next tp_batch_run, once that run's
 * kernel is queued and the host has seen the previous kernel finish (or in tp_synchronize /
 * tp_batch_download_gathered), so that no stream waits for another stream's event on the device.  Returns
 * at once; tp_synchronize (or tp_batch_download_gathered) waits for the gather.  Gathers complete in the
 * order they were requested; tp_batch_download always reads the results of the last run. */
int tp_batch_gather_async(tp_batch_t b, int root);
int tp_batch_download_gathered(tp_batch_t b, double* weights_all, int32_t* status_all); /* root only */

#ifdef __cplusplus
}
#endif
#endif /* TANGENCY_POSTERIOR_H */
