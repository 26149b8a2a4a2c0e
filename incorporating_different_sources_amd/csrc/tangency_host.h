// tangency_host.h - internal to the host layer of libtangency.so (tangency_api.cpp, tangency_sweep.cpp,
// tangency_plan.cpp, tangency_comm.cpp, tangency_replay.cpp): the handle and batch structures and the helpers the files share.
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <cstdint>
#include <initializer_list>
#include <string>
#include <vector>

#include "../../include/tangency_posterior.h"
#include "host_resources.h"
#include "posterior_kernels.h"
#include "posterior_grid_sweep.h"
#include "posterior_grid_sweep_tiled.h"
#include "posterior_prior_sweep.h"
#include "posterior_size_sweep.h"
#include "posterior_size_sweep_tiled.h"
#include "posterior_solve_sweep_tiled.h"
#include "posterior_window_sweep.h"

#include "backtest_replay.h"
#include "replay_summary.h"
#include "sweep_finish.h"
#include "posterior_spectral.h"

#define TP_REGION_MAX_STEPS 512

// Backtest replay (tp_replay_run / tp_replay_run_batch / tp_replay_download, tangency_replay.cpp): the inputs and results of
// the last run.  The replay belongs to the handle, not to a batch (tp_replay_run_batch reads a batch's results where they lie
// and keeps no pointer to them); plain DevBufs, freed with the handle.
struct ReplayWs {
    DevBuf S, rf, reb, weights, cols, caps, prev, next, port, order;
    DevBuf patch_date, patch_rows;  // tp_replay_run_batch: the patches' dates [n_patch] and rows [n_patch x patch_ld]
    DevBuf ret, turnover, metrics, status, bad_day;
    int64_t P = 0, D = 0, R = 0;    // shape of the last run
    bool ran = false;               // a run completed its launches (tp_replay_download has something to copy)
    // tp_replay_summary / tp_replay_download_summary (replay_summary.hip): the costs, the excess risk-free rates, the
    // rebalancing date of every trading day, and the records and statuses of the last summary [P x C]
    DevBuf sum_cost, sum_rf, sum_day, sum_stats, sum_status;
    std::vector<int32_t> h_reb;     // host copy of reb_day of the last run (the summary's table of days is built from it)
    int32_t C = 0;                  // costs of the last summary
    bool summarised = false;        // a summary of the last run completed its launch
};

// Members are destroyed in reverse order of declaration: the kernel stream is declared before every other stream and
// event, so it goes last (destroy_handle takes the communicator down before any of them).
struct tp_handle_s {
    int device = -1;
    Stream stream;
    Span kernel_span;               // the last timed launch outside a region (also: a synchronous upload, a download)
    Span region_span;               // tp_region_begin .. tp_region_end
    hipDeviceProp_t prop;
    std::string err;
    double kernel_ms = 0, h2d_ms = 0, d2h_ms = 0, gather_ms = 0;
    tp_launch_info_t last_launch{0, 0, 0, 0};
    ncclComm_t comm = nullptr;
    int rank = 0, world = 1;
    // overlapped gather (tp_batch_gather_async): its own high-priority stream next to the kernel stream
    Stream comm_stream;
    Span gather_span;
    // asynchronous uploads (tp_batch_upload_async): a copy stream of their own, so that the H2D copies of the next
    // batch run under the kernel of the current one
    Stream copy_stream;
    Span copy_span;
    tp_batch_t deferred = nullptr;  // batch whose tp_batch_gather_async is requested but not yet on the gather stream
    // Tuning switches (A/B measurements, tests): read from the environment ONCE, in tp_create, and changed only through
    // tp_set_option on this handle - no launch path reads the environment (several host threads launch at once in the
    // one-process-all-GPUs mode while a test may be changing it).
    tp_kopts_t opts{};
    int shared_tables = -1;         // "shared_tables": the Q tables of the register-tile path from one kernel (1), from the pair
                                    // (0), or the one kernel where it measured faster (-1); read by every run (tp_kargs_t)
    int no_shared_gram = 0;         // TP_NO_SHARED_GRAM / "no_shared_gram"
    int hf_share_min_blocks = 6;    // "hf_share_min_blocks": whole intraday blocks per window from which the large-k path shares them
    int tiled_arena_gib = 0;        // TP_TILED_ARENA_GIB / "tiled_arena_gib" (0: default)
    int tiled_arena_mib = 0;        // TP_TILED_ARENA_MIB / "tiled_arena_mib": a sub-GiB arena (tests: many sub-batches from few windows)
    int sweep_chunk_windows = 0;    // "sweep_chunk_windows": windows per sub-range of tp_batch_solve_sweep / _prior_sweep / _size_sweep / _window_sweep / _grid_sweep (0: automatic)
    int phase_limit = 0;            // TP_PHASE_LIMIT (diagnostic builds only)
    std::vector<tp_batch_t> batches;   // live batches of this handle (destroyed with it if the caller forgot them)
    // per-step kernel times inside a tp_region_begin / tp_region_end bracket: every timed launch of the region records
    // its own span (no host wait in between), tp_region_end reads them all (tp_region_steps returns them)
    std::vector<Span> ring;         // TP_REGION_MAX_STEPS spans, created whole or not at all
    int ring_used = 0;
    bool in_region = false;
    std::vector<double> step_ms;
    ReplayWs replay;                // tp_replay_run / tp_replay_download (destroy_handle drains the stream before it goes)
};

struct PriceStaging { DevBuf prices, num, den; };   // price front-end: prices and the row pairs of the returns

// Every sweep family has buffers of its own, so that a sweep leaves the batch's results, kept matrices and kept right-hand
// sides alone - and the other families' results: each download returns what its own last sweep wrote.  Plain DevBufs, freed
// with the batch (destroy_batch drains the streams first), declared - and so freed - in the order they always were.

// Solve sweeps.  `post` holds the matrices of ONE sub-range of windows at a time.
struct SolveSweepWs {
    DevBuf weights, status, aux;    // outputs of the run kernel that serves as the Gram pass (tp_batch_solve_sweep)
    DevBuf rhs0, post;              // every window's default right-hand side [W x k]; kept matrices [chunk x k x k]
    DevBuf shift, rhs, x, xstatus;  // the caller's shifts and right-hand sides; solutions and their statuses
    // tp_batch_solve_sweep_tiled: its own workspace of (window, shift) entries at the sweep's geometry (KP from k + R) - the
    // batch's run workspace keeps the size and shape tp_batch_run gives it
    DevBuf arena, rinv, flags;
    DevBuf part;                    // tp_batch_size_sweep_tiled borrows that workspace (R = n_size): pieces of its prior products
    int S = 0, R = 0;               // shape of the last sweep (0: none yet)
    bool default_rhs = false;       // the last sweep solved for the default right-hand side (slot 0 of its R columns)
    // tp_batch_sweep_finish (sweep_finish.hip): the uploaded scalars n [W], kappa [W] and (xi, eta) [W x S x 2], the groups'
    // partial sums [W x NG x k] and statuses [W x NG], and the results weights [W x k], status [W], aux [W x S x 4]
    DevBuf fin_n, fin_kappa, fin_hyper, fin_part, fin_gstatus, fin_weights, fin_status, fin_aux;
    bool finished = false;          // a finish of the LAST sweep completed its launches (a new sweep clears it)
    bool finish_stale = false;      // there was a finish, and a later sweep replaced the solutions it read
};

// Spectral ridge sweep (`sp`, tp_batch_spectral_greyserman, posterior_spectral.hip): buffers of its own throughout - the outputs
// of the run kernel that serves as its Gram pass included -, so that it leaves runs, solve sweeps and a sweep finish alone.
struct SpectralWs {
    DevBuf gw, gs, ga;              // outputs of the run kernel that serves as the Gram pass
    DevBuf t, post;                 // every window's t [W x k]; the matrices [chunk x k x k] of ONE sub-range at a time
    DevBuf V;                       // eigenvectors: [chunk x k x k] of one sub-range, or [W x k x k] (keep_vectors)
    DevBuf lambda, that, ohat;      // [W x k] each
    DevBuf sweeps, jstatus;         // [W] Jacobi sweeps and the eigensolver's own status
    DevBuf n, kappa, hyper;         // the uploaded scalars n [W], kappa [W] and (xi, eta) [W x S x 2]
    DevBuf part, gstatus;           // the groups' partial sums [W x NG x k] and statuses [W x NG]
    DevBuf weights, status, aux;    // the results: [W x k], [W], [W x S x 4]
    int S = 0;                      // draws of the last call (0: none yet)
    bool kept_vectors = false;      // the last call kept V of every window
};

// Prior sweeps (`ps`) and the size sweep (`zs`): one type, two instances - a size sweep must not disturb what
// tp_batch_download_prior_sweep returns, and the reverse.  C / T hold the matrices of ONE sub-range at a time: the intraday
// scatters and daily Grams (a Jeffreys size sweep: M in T, no C).
struct PriorSweepWs {
    DevBuf C, T, t, n0, w0;
    DevBuf sizes;                   // size sweep: the universes' sizes [S]
    DevBuf weights, status, aux;
    DevBuf gw, gs, ga;              // Jeffreys size sweep: outputs of the run kernel that serves as its Gram pass
    int P = 0, S = 0;               // shape of the last sweep (0: none yet; a prior sweep has S = 1)
};

// Window sweep (`wn`).  C / T hold the matrices of ONE sub-range at a time: one intraday scatter (conjugate) and L snapshots
// of the daily Gram per window; t, the delta sums and the results cover the batch.
struct WindowSweepWs {
    DevBuf C, T, t, n0, w0;
    DevBuf N, rows;                 // the lengths' N [L] and row counts [W x L]
    DevBuf delta, dv, ds;           // the caller's row offsets [W x L x n_r]; their sums v [W x L x k] and (s1, s2) [W x L x 2]
    DevBuf weights, status, aux;
    // tp_batch_window_sweep_tiled: C w0 [chunk x P x k] and w0'C w0 [chunk x P] of one sub-range; the results of one group of
    // arena entries (one length) as tp_tiled_factor_launch writes them, before they go to their slots
    DevBuf cw, cq, stage_w, stage_s, stage_a;
    int P = 0, L = 0;               // shape of the last sweep (0: none yet)
};

// Grid sweep (`gr`): the window sweep's buffers - C, the snapshots, the delta sums, the results at [W x P x L x S] - of its
// own, so that tp_batch_download_window_sweep returns what it returned before, and the universes' sizes.
struct GridSweepWs : WindowSweepWs {
    DevBuf sizes;                   // [S]
    DevBuf mdiag;                   // tp_batch_grid_sweep_tiled: the diagonals [entries of one group x k] its fill keeps for the statuses
                                    // (its prior products of one sub-range lie in cw [chunk x P x S x k] and cq [chunk x P x S])
    int S = 0;                      // sizes of the last sweep (0: none yet)
};

struct tp_batch_s {
    tp_handle_t h = nullptr;
    tp_params_t p{};
    int64_t W = 0;
    int panel_ld = 0, hf_ld = 0;
    DevBuf panel, start, row_idx, n_rows, col_idx, rf_adj, hf_panel, hf_start, hf_row_idx, hf_count, w0, n0;
    DevBuf weights, status, aux, dbg, gather_w, gather_s, weights2, status2, stamps, rhs, out_rhs, shift;
    DevBuf post;                                              // kept posterior matrices [post_count x k x k] (tp_batch_keep_posterior)
    int64_t post_w0 = 0, post_count = 0;
    SolveSweepWs sw;                                          // tp_batch_solve_sweep / _solve_sweep_tiled
    SpectralWs sp;                                            // tp_batch_spectral_greyserman
    PriorSweepWs ps, zs;                                      // tp_batch_prior_sweep / _prior_sweep_tiled; tp_batch_size_sweep / _size_sweep_tiled
    WindowSweepWs wn;                                         // tp_batch_window_sweep / _window_sweep_tiled
    GridSweepWs gr;                                           // tp_batch_grid_sweep / _grid_sweep_tiled
    PriceStaging fe, fe_hf;                                   // daily and intraday (freed after a synchronous upload)
    DevBuf prefix;                                            // shared Gram prefixes of the daily panel (register-tile path)
    int prefix_nblk = 0;                                      // > 0: the layout qualifies (decided at upload)
    int winsum_L[4] = {0, 0, 0, 0};                           // register-tile path: the whole-block counts of the windows
    bool winsum_zero = false;                                 // register-tile path: the tables end in an all-zero slot and the
                                                              // batch may start its accumulators from a slot (plan_shared_gram)
    DevBuf t_arena, t_rinv, t_ybar, t_zc, t_scal, t_flags;    // large-k path workspace
    // large-k path, conjugate: shared intraday sums (posterior_tiled_wave.h).  Decided at upload (plan_shared_hf): the
    // windows' intraday rows are contiguous, of one length, and advance by hf_B rows; the tables are per sub-batch
    // large-k path: the daily tables cover the blocks of the sub-batch in flight (plan_daily_tables); host copies of
    // what the block ranges are computed from
    bool prefix_per_sub = false;
    std::vector<int64_t> h_start;
    std::vector<int32_t> h_n_rows;
    std::vector<int64_t> h_hf_start;                          // host copy of hf_start (the sub-batches' block ranges)
    int hf_B = 0, hf_L = 0;                                   // rows per block (0 = not shared), whole blocks per window
    long long hf_phase = 0;                                   // blocks start at rows = hf_phase (mod hf_B)
    DevBuf hf_prefix;                                         // block Grams + block-window sums of the sub-batch in flight
    DevBuf t_part;                                            // pieces of S0 w0 per (window, row block, column block)
    int64_t tiled_capacity = 0;                               // windows in flight per sub-batch
    bool uploaded = false;
    bool has_run = false;                            // a tp_batch_run queued its launches: (out_weights, out_status) hold results
    bool gathered = false;
    bool rhs_valid = false;                          // out_rhs was allocated before the last run (tp_batch_keep_rhs)
    bool post_valid = false;                         // post was allocated before the last run (tp_batch_keep_posterior)
    Event ran;                                       // end of this batch's last launch (recorded by every tp_batch_run)
    Event upload_done;                               // tp_batch_upload_async: end of the copies on the copy stream
    bool upload_pending = false;
    // tp_batch_gather_async: results alternate between (weights, status) and (weights2, status2), so that the
    // gather of run i reads one pair while run i+1 writes the other; run i+2 waits for that gather's event
    bool pingpong = false;
    int parity = 0;                                  // pair written by the last run
    Event gather_done[2];
    bool gather_pending[2] = {false, false};
    Event snap;                                      // end of the run whose results the requested gather reads
    bool gather_req = false;                         // requested by tp_batch_gather_async, issued by flush_gather
    int gather_req_parity = 0, gather_root = 0;
    double* out_weights() const { return (double*)(parity ? weights2.p : weights.p); }
    int32_t* out_status() const { return (int32_t*)(parity ? status2.p : status.p); }
};

namespace tp_host {

// records the message on the handle (h = NULL: for tp_last_error(NULL)) and returns `code`
int fail(tp_handle_t h, int code, const char* fmt, ...);

#define HIP_TRY(h, expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) \
    return tp_host::fail((h), TP_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); } while (0)
#define NCCL_TRY(h, expr) do { ncclResult_t r_ = (expr); if (r_ != ncclSuccess) \
    return tp_host::fail((h), TP_ERR_RCCL, "%s failed: %s (%s:%d)", #expr, ncclGetErrorString(r_), __FILE__, __LINE__); } while (0)

// the one way to allocate device memory: grow-only, names what could not be had
int ensure(tp_handle_t h, DevBuf& b, size_t bytes, const char* what);

inline int harvest_kernel_time(tp_handle_t h) {
    HIP_TRY(h, h->kernel_span.read(h->kernel_ms));
    return TP_OK;
}

// drain the kernel stream, read the kernel span, copy what has a destination, drain
struct Copy { void* dst; const void* src; size_t bytes; };
int download(tp_handle_t h, std::initializer_list<Copy> copies);

// tangency_api.cpp: what the sweeps (tangency_sweep.cpp) launch and time with
tp_kargs_t make_kargs(tp_batch_t b);                   // the batch as tp_batch_run launches it
int launch(tp_batch_t b, const tp_kargs_t& a, int64_t count, bool timed);
// The span a timed launch uses: inside a region the next slot of the ring (read by tp_region_end) while slots remain,
// the handle's kernel span otherwise.
Span& timed_span(tp_handle_t h);
int timed_done(tp_handle_t h, Span& span);             // the end of what timed_span(h) brackets; a ring slot is used up
int begin_launches(tp_batch_t b);                      // before and after the launches of a tp_batch_run or a sweep
int end_launches(tp_batch_t b);

// tangency_plan.cpp: input validation, upload planning, large-k launch planning
int validate_pairs(tp_handle_t h, const char* what, const int32_t* num, const int32_t* den, int64_t n, int64_t price_rows);
int validate_inputs(tp_handle_t h, const tp_params_t& p, int64_t W, const tp_inputs_t* in_raw);
// entries a tiled arena of `per_entry` bytes each may hold: the budget is 32 GiB, never more than a third
// of what is free (`held` bytes, about to be reallocated, count as free), tiled_arena_gib / _mib override it; 1 .. 65,535
int64_t tiled_arena_entries(tp_handle_t h, size_t per_entry, size_t held = 0);
// `entries`: arena slots a caller other than a run could fill at once (the tiled prior sweep: (window, prior) pairs); the
// workspace holds up to max(W, entries) of them where the arena budget allows
int ensure_tiled_ws(tp_batch_t b, tp_tiled_ws_t* ws, int64_t entries = 0);
int plan_daily_tables(tp_batch_t b, tp_kargs_t& sub);
int plan_hf_tables(tp_batch_t b, tp_kargs_t& sub);
int plan_shared_gram(tp_batch_t b, const tp_inputs_t* in, hipStream_t st);
void plan_shared_hf(tp_batch_t b, const tp_inputs_t* in);

// tangency_comm.cpp
int flush_gather(tp_handle_t h);

}  // namespace tp_host
