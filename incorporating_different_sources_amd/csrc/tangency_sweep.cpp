// tangency_sweep.cpp - the sweeps of the C-ABI of libtangency.so (include/tangency_posterior.h): many solves per window
// from one Gram pass - tp_batch_solve_sweep, _prior_sweep, _size_sweep, _window_sweep, _grid_sweep, the five tiled forms above
// tp_sweep_max_assets(), the sweep finish and the spectral ridge sweep (tp_batch_spectral_greyserman), and their downloads.  Every sweep is: checks, a drain of the handle's stream, its workspace (SolveSweepWs / PriorSweepWs,
// tangency_host.h), then per sub-range of windows a Gram stage and a solve stage inside one timed span.
#include <cmath>
#include <cstring>
#include <algorithm>
#include <string>
#include <vector>

#include "tangency_host.h"

using namespace tp_host;

// Bound of the matrices one sub-range of windows keeps: 256 MiB, the size of the Infinity Cache (the solve kernel reads what
// the Gram pass has just written).
#define TP_SWEEP_WORKSPACE_BYTES (256ull << 20)
// tp_batch_window_sweep_tiled (and tp_batch_grid_sweep_tiled, which keeps its rule): 4 GiB.  Its entries are factorised in groups of ONE length, each a chain of some 3 NS small
// launches over the sub-range's windows x priors, so the sub-range - not the cache - decides how full the chip runs: at 256 MiB
// (25 windows at k = 500, L = 4) the sweep took 1.6 - 3.6x the device time of one batch per length, at 4 GiB 1.3 - 2.5x less
// (DESIGN.md section 4m).
#define TP_WINDOW_SWEEP_TILED_WORKSPACE_BYTES (4096ull << 20)

namespace {

// ---- what the sweeps share ---------------------------------------------------------------------------------------------

// the sweep kernels serve k <= tp_sweep_max_assets(), the tiled forms (`partner`: the sweep below them) the universes above
int check_sweep_k(tp_handle_t h, bool tiled, const char* name, const char* partner, int k) {
    if (!tiled && k > tp_sweep_max_assets())
        return fail(h, TP_ERR_UNSUPPORTED, "%s: k=%d exceeds the sweep kernel's largest universe %d", name, k, tp_sweep_max_assets());
    if (tiled && k <= tp_sweep_max_assets())
        return fail(h, TP_ERR_UNSUPPORTED, "%s: k=%d is served by %s (k <= %d)", name, k, partner, tp_sweep_max_assets());
    return TP_OK;
}

// a[0 .. n) of the caller: every entry finite and >= 0 (`positive`: > 0)
int check_finite_sign(tp_handle_t h, const char* name, const char* what, const double* a, int64_t n, bool positive) {
    for (int64_t i = 0; i < n; ++i)
        if (!std::isfinite(a[i]) || a[i] < 0.0 || (positive && a[i] == 0.0))
            return fail(h, TP_ERR_INVALID, "%s: %s[%lld] must be finite and %s", name, what, (long long)i, positive ? "> 0" : ">= 0");
    return TP_OK;
}

// Unlike tp_batch_run a sweep drains the handle's stream before it starts (documented in the header): an earlier launch may
// still use the buffers (and the tiled workspace) about to be reallocated or refilled, and the kernel span may still be
// waiting to be read
int drain_for_sweep(tp_batch_t b) {
    tp_handle_t h = b->h;
    int rc = begin_launches(b);
    if (rc != TP_OK) return rc;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return harvest_kernel_time(h);
}

// Windows per sub-range: the "sweep_chunk_windows" option, else as many as `budget` bytes hold at `bytes_per_window`
// of kept matrices; never more than 2^30 (window, shift) or (window, prior) pairs per launch; within [1, W].
// clamp_option_to_workspace = false, the plain solve sweep only: its option is documented as overriding the workspace bound
// (tp_set_option in the header); the later sweeps honour it below the bound.
int64_t sweep_chunk(tp_handle_t h, size_t bytes_per_window, int64_t pairs_per_window, int64_t W, bool clamp_option_to_workspace,
                    size_t budget = TP_SWEEP_WORKSPACE_BYTES) {
    const int64_t fit = (int64_t)(budget / bytes_per_window);
    int64_t chunk = h->sweep_chunk_windows > 0 ? h->sweep_chunk_windows : fit;
    if (clamp_option_to_workspace) chunk = std::min(chunk, fit);
    chunk = std::min(chunk, ((int64_t)1 << 30) / pairs_per_window);
    return std::min(std::max<int64_t>(chunk, 1), W);
}

// The batch as a plain run would see it, with nothing attached: no custom right-hand side, no shift, no shared daily or
// intraday block sums (whether those are used depends on W: a sweep's matrices must not), no stamps, no outputs.  A sweep's
// Gram stage sets what it adds.
tp_kargs_t neutral_kargs(tp_batch_t b) {
    tp_kargs_t a = make_kargs(b);
    a.rhs = nullptr; a.shift = nullptr;
    a.prefix = nullptr; a.winsum = nullptr; a.prefix_nblk = 0; a.prefix_blk0 = 0;
    for (int i = 0; i < 4; ++i) a.winsum_L[i] = 0;
    a.hf_prefix = nullptr; a.hf_winsum = nullptr;
    a.weights = nullptr; a.status = nullptr; a.aux = nullptr;
    a.out_rhs = nullptr; a.out_post = nullptr; a.post_count = 0;
    a.stamps = nullptr;
    return a;
}

int launched(tp_handle_t h, hipError_t e, const char* what) {
    return e == hipSuccess ? TP_OK : fail(h, TP_ERR_HIP, "%s launch failed: %s", what, hipGetErrorString(e));
}

// f(first, count) over [0, total) in groups of at most `step`; stops at the first error
template <class F>
int in_groups(int64_t total, int64_t step, F f) {
    for (int64_t i0 = 0; i0 < total; i0 += step) {
        const int rc = f(i0, std::min(step, total - i0));
        if (rc != TP_OK) return rc;
    }
    return TP_OK;
}

// The launches of a sweep, body(w0, n) per sub-range of `chunk` windows, inside ONE span: a sweep is one step of
// tp_region_steps, kernel_ms = all its launches.  tp_last_launch keeps describing tp_batch_run launches, whatever the body
// launched and however it ended.  set_shape() records the sweep's shape for its download - after success only.
template <class Body, class SetShape>
int run_sweep(tp_batch_t b, int64_t chunk, Body body, SetShape set_shape) {
    tp_handle_t h = b->h;
    const tp_launch_info_t keep_launch = h->last_launch;
    Span& span = timed_span(h);
    HIP_TRY(h, span.begin(h->stream));
    int rc = in_groups(b->W, chunk, body);
    h->last_launch = keep_launch;
    if (rc == TP_OK) rc = timed_done(h, span);
    if (rc != TP_OK) return rc;
    set_shape();
    return end_launches(b);                            // (the sweep reads the batch's inputs and writes none of its results)
}

// Tiled sweeps: the Gram stage of the batch's own tiled pipeline over the windows [w0, w0 + n) of a sub-range, every pass of
// `passes` per group of as many windows as the run workspace holds (`cap`); the kept-matrix store covers the sub-range
int tiled_gram_stage(tp_batch_t b, const char* what, std::initializer_list<tp_kargs_t*> passes, const tp_tiled_ws_t& ws, int64_t cap,
                     int64_t w0, int64_t n) {
    return in_groups(n, cap, [&](int64_t g0, int64_t ng) {
        for (tp_kargs_t* g : passes) {
            g->w_first = w0 + g0; g->w_count = ng;
            g->post_w0 = w0; g->post_count = n;
            const int rc = launched(b->h, tp_tiled_gram_launch(*g, ws, b->h->stream, false), what);
            if (rc != TP_OK) return rc;
        }
        return TP_OK;
    });
}

// ---- solve sweeps -----------------------------------------------------------------------------------------------------

// What the two solve sweeps share - tp_batch_solve_sweep (`tiled` = false, k <= tp_sweep_max_assets()) and
// tp_batch_solve_sweep_tiled (above it): the argument checks, the drain, the windows per sub-range (one k x k matrix per
// window), the sweep's buffers and the copies of the caller's arrays.  *chunk_out = 0: W = 0, nothing to launch (the shape is set).
int solve_sweep_prepare(tp_batch_t b, const char* name, bool tiled, int32_t n_shift, const double* shift, int32_t n_rhs,
                        const double* rhs, int32_t default_rhs, int* S_out, int* R_out, int64_t* chunk_out) {
    tp_handle_t h = b->h;
    SolveSweepWs& ws = b->sw;
    const int k = b->p.k;
    const int64_t W = b->W;
    *chunk_out = 0;
    if (!b->uploaded) return fail(h, TP_ERR_INVALID, "%s before tp_batch_upload", name);
    if (n_shift < 0) return fail(h, TP_ERR_INVALID, "%s: n_shift=%d < 0", name, n_shift);
    if (n_rhs < 0) return fail(h, TP_ERR_INVALID, "%s: n_rhs=%d < 0", name, n_rhs);
    if (shift && b->p.strategy != TP_STRATEGY_JEFFREYS)
        return fail(h, TP_ERR_INVALID, "%s: a shift applies to the Jeffreys strategy only", name);
    if (shift && n_shift < 1) return fail(h, TP_ERR_INVALID, "%s: shift given with n_shift=0", name);
    if (!shift && n_shift > 1) return fail(h, TP_ERR_INVALID, "%s: n_shift=%d without shift", name, n_shift);
    const int S = n_shift > 1 ? n_shift : 1;
    const long long R = (default_rhs ? 1 : 0) + (long long)n_rhs;
    if (R < 1 || R > TP_SWEEP_MAX_RHS)
        return fail(h, TP_ERR_INVALID, "%s: %lld right-hand sides per window outside [1, %d]", name, R, TP_SWEEP_MAX_RHS);
    if (n_rhs > 0 && !rhs) return fail(h, TP_ERR_INVALID, "%s: n_rhs=%d without rhs", name, n_rhs);
    int rc = shift ? check_finite_sign(h, name, "shift", shift, 2 * W * S, false) : TP_OK;
    if (rc == TP_OK) rc = check_sweep_k(h, tiled, name, "tp_batch_solve_sweep", k);
    if (rc != TP_OK) return rc;
    if (tiled && k + R > tp_max_assets() + 1)
        return fail(h, TP_ERR_UNSUPPORTED, "%s: k=%d with %lld right-hand sides exceeds the arena side %d", name, k, R, tp_max_assets() + 1);
    rc = drain_for_sweep(b);
    if (rc != TP_OK) return rc;
    ws.S = 0; ws.R = 0;
    if (ws.finished) { ws.finished = false; ws.finish_stale = true; }   // (a finish read the solutions about to be replaced)
    ws.default_rhs = default_rhs != 0;
    *S_out = S; *R_out = (int)R;
    if (W == 0) { ws.S = S; ws.R = (int)R; return TP_OK; }
    const size_t mat_bytes = sizeof(double) * (size_t)k * k;
    const int64_t chunk = sweep_chunk(h, mat_bytes, S, W, tiled);
    const std::string what = std::string(name) + ": ";
    rc = ensure(h, ws.post, mat_bytes * (size_t)chunk, (what + "kept matrices of one sub-range").c_str());
    if (!tiled) {                                      // outputs of the run kernel that serves as the Gram pass
        if (rc == TP_OK) rc = ensure(h, ws.weights, sizeof(double) * (size_t)W * k, (what + "weights of the Gram pass").c_str());
        if (rc == TP_OK) rc = ensure(h, ws.status, sizeof(int32_t) * (size_t)W, (what + "statuses of the Gram pass").c_str());
        if (rc == TP_OK) rc = ensure(h, ws.aux, sizeof(double) * (size_t)W * TP_AUX_STRIDE, (what + "aux of the Gram pass").c_str());
    }
    if (rc == TP_OK) rc = ensure(h, ws.rhs0, sizeof(double) * (size_t)W * k, (what + "default right-hand sides").c_str());
    if (rc == TP_OK) rc = ensure(h, ws.x, sizeof(double) * (size_t)W * S * (size_t)R * k, (what + "solutions").c_str());
    if (rc == TP_OK) rc = ensure(h, ws.xstatus, sizeof(int32_t) * (size_t)W * S, (what + "solution statuses").c_str());
    if (rc == TP_OK && shift) rc = ensure(h, ws.shift, sizeof(double) * 2 * (size_t)W * S, (what + "shifts").c_str());
    if (rc == TP_OK && n_rhs > 0) rc = ensure(h, ws.rhs, sizeof(double) * (size_t)W * n_rhs * k, (what + "right-hand sides").c_str());
    if (rc != TP_OK) return rc;
    // the caller's arrays: copied here, no host pointer is kept
    if (shift) HIP_TRY(h, hipMemcpyAsync(ws.shift.p, shift, sizeof(double) * 2 * (size_t)W * S, hipMemcpyHostToDevice, h->stream));
    if (n_rhs > 0) HIP_TRY(h, hipMemcpyAsync(ws.rhs.p, rhs, sizeof(double) * (size_t)W * n_rhs * k, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));       // the copies are done when the call returns, pinned host memory or not
    *chunk_out = chunk;
    return TP_OK;
}

// The sweep's own tiled workspace (arena, inverse diagonal blocks, flags) at the sweep's geometry, KP from k + R: as many
// (window, shift) entries as the large-k arena budget allows (tiled_arena_entries, the rule ensure_tiled_ws sizes by; what this
// workspace already holds counts as free), at most `entries`.  The batch's run workspace is left as it is.  `part_doubles` > 0
// (the tiled size sweep): that many doubles of ws->part per entry, inside the same budget.
int ensure_sweep_tiled_ws(tp_batch_t b, int R, int64_t entries, tp_tiled_ws_t* ws, int64_t* cap_out, size_t part_doubles = 0) {
    tp_handle_t h = b->h;
    SolveSweepWs& sw = b->sw;
    int KP, NS, NSB;
    tp_solve_sweep_tiled_geometry(b->p.k, R, &KP, &NS, &NSB);
    const size_t per_entry = sizeof(double) * ((size_t)KP * KP + (size_t)NSB * 64 * 64 + part_doubles) + sizeof(int);
    int64_t G = tiled_arena_entries(h, per_entry, sw.arena.bytes + sw.rinv.bytes + sw.flags.bytes + sw.part.bytes);
    if (G > entries) G = entries;
    int rc = ensure(h, sw.arena, sizeof(double) * (size_t)G * KP * KP, "tp_batch_solve_sweep_tiled: arena");
    if (rc == TP_OK) rc = ensure(h, sw.rinv, sizeof(double) * (size_t)G * NSB * 64 * 64, "tp_batch_solve_sweep_tiled: inverse diagonal blocks");
    if (rc == TP_OK) rc = ensure(h, sw.flags, sizeof(int) * (size_t)G, "tp_batch_solve_sweep_tiled: flags");
    if (rc == TP_OK && part_doubles > 0) rc = ensure(h, sw.part, sizeof(double) * (size_t)G * part_doubles, "tp_batch_size_sweep_tiled: prior products");
    if (rc != TP_OK) return rc;
    memset(ws, 0, sizeof *ws);
    ws->arena = (double*)sw.arena.p; ws->rinv = (double*)sw.rinv.p; ws->flags = (int*)sw.flags.p;
    if (part_doubles > 0) ws->part = (double*)sw.part.p;
    ws->KP = KP; ws->NS = NS; ws->NSB = NSB;
    *cap_out = G;
    return TP_OK;
}

// ---- prior sweeps and the size sweep ------------------------------------------------------------------------------------

// What the prior sweeps and the size sweep share - tp_batch_prior_sweep (`tiled` = false, k <= tp_sweep_max_assets()),
// tp_batch_prior_sweep_tiled (above it), tp_batch_size_sweep and tp_batch_size_sweep_tiled (`sz` given: n_size universes per
// (window, prior), a Jeffreys batch allowed - without priors; the two share `zs`), each on the workspace `ws` of its own: the
// argument checks, the k range, the drain, the windows per
// sub-range (C and T: two k x k matrices per window), the sweep's buffers and the copies of the caller's arrays.
// *chunk_out = 0: W = 0, nothing to launch (the sweep's shape is set).
struct SizeAxis { int32_t n_size; const int32_t* sizes; };

int check_size_axis(tp_handle_t h, const char* name, const SizeAxis& sz, int k) {
    if (sz.n_size < 1 || sz.n_size > TP_SWEEP_MAX_RHS)
        return fail(h, TP_ERR_INVALID, "%s: n_size=%d outside [1, %d]", name, sz.n_size, TP_SWEEP_MAX_RHS);
    if (!sz.sizes) return fail(h, TP_ERR_INVALID, "%s: sizes is NULL", name);
    for (int s = 0; s < sz.n_size; ++s)
        if (sz.sizes[s] < 1 || sz.sizes[s] > k || (s > 0 && sz.sizes[s] <= sz.sizes[s - 1]))
            return fail(h, TP_ERR_INVALID, "%s: sizes[%d]=%d: strictly increasing sizes within [1, %d] expected", name, s, sz.sizes[s], k);
    return TP_OK;
}

// w0 [pairs x S x k] of the caller (`sz` == nullptr: S = 1): finite - with sizes, inside each vector's prefix only (a size sweep
// reads the first sizes[s] entries of a vector)
int check_finite_w0(tp_handle_t h, const char* name, const double* w0, int64_t pairs, int k, const SizeAxis* sz) {
    const int S = sz ? sz->n_size : 1;
    for (int64_t e = 0; e < pairs * S; ++e) {
        const int ke = sz ? sz->sizes[e % S] : k;
        for (int i = 0; i < ke; ++i)
            if (!std::isfinite(w0[e * k + i])) return fail(h, TP_ERR_INVALID, "%s: w0[%lld] must be finite", name, (long long)(e * k + i));
    }
    return TP_OK;
}
int prior_sweep_prepare(tp_batch_t b, PriorSweepWs& ws, const char* name, bool tiled, int32_t n_prior, const double* n0,
                        const double* w0, int64_t* chunk_out, const SizeAxis* sz = nullptr) {
    tp_handle_t h = b->h;
    const int k = b->p.k;
    const int64_t W = b->W;
    *chunk_out = 0;
    const bool conj = b->p.strategy == TP_STRATEGY_CONJUGATE;
    if (!sz && !conj) return fail(h, TP_ERR_INVALID, "%s applies to the conjugate strategy only", name);
    if (!b->uploaded) return fail(h, TP_ERR_INVALID, "%s before tp_batch_upload", name);
    if (sz) {
        const int rcs = check_size_axis(h, name, *sz, k);
        if (rcs != TP_OK) return rcs;
    }
    if (sz && !conj && (n_prior != 0 || n0 || w0))
        return fail(h, TP_ERR_INVALID, "%s: a Jeffreys batch takes no priors (n_prior = 0, n0 = w0 = NULL)", name);
    const int P = conj ? n_prior : 1;
    const int S = sz ? sz->n_size : 1;
    int rc = TP_OK;
    if (conj) {
        if (n_prior < 1) return fail(h, TP_ERR_INVALID, "%s: n_prior=%d < 1", name, n_prior);
        if (!n0 || !w0) return fail(h, TP_ERR_INVALID, "%s: %s is NULL", name, !n0 ? "n0" : "w0");
        rc = check_finite_sign(h, name, "n0", n0, W * P, true);
        if (rc != TP_OK) return rc;
        rc = check_finite_w0(h, name, w0, W * P, k, sz);
        if (rc != TP_OK) return rc;
    }
    rc = check_sweep_k(h, tiled, name, sz ? "tp_batch_size_sweep" : "tp_batch_prior_sweep", k);
    if (rc != TP_OK) return rc;
    if (tiled && sz && k + S > tp_max_assets() + 1)
        return fail(h, TP_ERR_UNSUPPORTED, "%s: k=%d with %d sizes exceeds the arena side %d", name, k, S, tp_max_assets() + 1);
    rc = drain_for_sweep(b);
    if (rc != TP_OK) return rc;
    ws.P = 0; ws.S = 0;
    if (W == 0) { ws.P = P; ws.S = S; return TP_OK; }
    const size_t mat_bytes = sizeof(double) * (size_t)k * k;
    const int64_t chunk = sweep_chunk(h, 2 * mat_bytes, P, W, true);
    const size_t WP = (size_t)W * (size_t)P;
    const size_t WPS = WP * (size_t)S;
    const std::string what = std::string(name) + ": ";
    if (conj) rc = ensure(h, ws.C, mat_bytes * (size_t)chunk, (what + "intraday scatters of one sub-range").c_str());
    if (rc == TP_OK) rc = ensure(h, ws.T, mat_bytes * (size_t)chunk, (what + (conj ? "daily Grams of one sub-range" : "matrices of one sub-range")).c_str());
    if (rc == TP_OK) rc = ensure(h, ws.t, sizeof(double) * (size_t)W * k, (what + "daily column sums").c_str());
    if (rc == TP_OK && conj) rc = ensure(h, ws.n0, sizeof(double) * WP, (what + "prior strengths").c_str());
    if (rc == TP_OK && conj) rc = ensure(h, ws.w0, sizeof(double) * WPS * k, (what + "prior weights").c_str());
    if (rc == TP_OK) rc = ensure(h, ws.weights, sizeof(double) * WPS * k, (what + "weights").c_str());
    if (rc == TP_OK) rc = ensure(h, ws.status, sizeof(int32_t) * WPS, (what + "statuses").c_str());
    if (rc == TP_OK) rc = ensure(h, ws.aux, sizeof(double) * WPS * TP_AUX_STRIDE, (what + "aux").c_str());
    if (rc == TP_OK && sz) rc = ensure(h, ws.sizes, sizeof(int32_t) * (size_t)S, (what + "sizes").c_str());
    if (rc == TP_OK && sz && !conj && !tiled) {            // outputs of the run kernel that serves as the Gram pass
        rc = ensure(h, ws.gw, sizeof(double) * (size_t)W * k, (what + "weights of the Gram pass").c_str());
        if (rc == TP_OK) rc = ensure(h, ws.gs, sizeof(int32_t) * (size_t)W, (what + "statuses of the Gram pass").c_str());
        if (rc == TP_OK) rc = ensure(h, ws.ga, sizeof(double) * (size_t)W * TP_AUX_STRIDE, (what + "aux of the Gram pass").c_str());
    }
    if (rc != TP_OK) return rc;
    // the caller's arrays: copied here, no host pointer is kept
    if (conj) {
        HIP_TRY(h, hipMemcpyAsync(ws.n0.p, n0, sizeof(double) * WP, hipMemcpyHostToDevice, h->stream));
        HIP_TRY(h, hipMemcpyAsync(ws.w0.p, w0, sizeof(double) * WPS * k, hipMemcpyHostToDevice, h->stream));
    }
    if (sz) HIP_TRY(h, hipMemcpyAsync(ws.sizes.p, sz->sizes, sizeof(int32_t) * (size_t)S, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));       // the copies are done when the call returns, pinned host memory or not
    *chunk_out = chunk;
    return TP_OK;
}

// Gram pass of a prior sweep or a conjugate size sweep (posterior_gram_nt.hip) over the windows [w0, w0 + n): the windows' rows
// as a plain run reads them, no prior; C and T of the sub-range and t go into `ws`
int gram_pass(tp_batch_t b, const char* name, const char* what, tp_gram_kargs_t& ga, int64_t w0, int64_t n) {
    ga.in.w_first = w0; ga.in.w_count = n;
    const hipError_t e = tp_gram_launch(ga, b->h->stream);
    if (e == hipErrorNotSupported)
        return fail(b->h, TP_ERR_UNSUPPORTED, "%s: windows of %d daily / %d intraday rows in the index layout are "
                                              "too long for the Gram pass", name, b->p.n_r, b->p.m);
    return launched(b->h, e, what);
}

tp_gram_kargs_t gram_pass_kargs(tp_batch_t b, const PriorSweepWs& ws) {
    tp_gram_kargs_t ga;
    memset(&ga, 0, sizeof ga);
    ga.in = neutral_kargs(b);
    ga.in.w0 = nullptr; ga.in.n0 = nullptr;
    ga.C = (double*)ws.C.p; ga.T = (double*)ws.T.p; ga.t = (double*)ws.t.p;
    return ga;
}

// The two passes of the batch's tiled Gram stage that give a conjugate tiled sweep its matrices, steered by their arguments: T
// and t (into the stores `T`, `t`) as a Jeffreys batch without centring over the daily rows, C as a Jeffreys batch centred by the window's row
// count over the INTRADAY rows
void tiled_conjugate_gram_kargs(tp_batch_t b, const DevBuf& T, const DevBuf& t, const DevBuf& C, tp_kargs_t* ta_out, tp_kargs_t* ca_out) {
    // T and t: the daily rows as a plain run reads them, uncentred and without the prior
    tp_kargs_t ta = neutral_kargs(b);
    ta.strategy = TP_STRATEGY_JEFFREYS;
    ta.center_rows = 2;
    ta.w0 = nullptr; ta.n0 = nullptr;
    ta.out_rhs = (double*)t.p;
    ta.out_post = (double*)T.p;
    // C: the same stage over the intraday rows - the daily-panel fields name the intraday panel (its own 32-bit offset flags:
    // make_kargs formed hf_off32 from that panel's bytes, leading dimension and m), centred by the window's row count
    tp_kargs_t ca = ta;
    ca.panel = ta.hf_panel; ca.start = ta.hf_start; ca.row_idx = ta.hf_row_idx; ca.n_rows = ta.hf_count;
    ca.n_r = b->p.m; ca.rf_adj = nullptr;
    ca.panel_ld = ta.hf_ld; ca.panel_off32 = ta.hf_off32;
    ca.center_rows = 1;
    ca.out_rhs = nullptr;
    ca.out_post = (double*)C.p;
    for (tp_kargs_t* g : {&ta, &ca}) { g->hf_panel = nullptr; g->hf_start = nullptr; g->hf_row_idx = nullptr; g->hf_count = nullptr; g->hf_off32 = 0; }
    *ta_out = ta; *ca_out = ca;
}

// the results of the last sweep on `ws`: [W x P x S] weight vectors, statuses and aux rows (W = 0: nothing to copy)
int download_prior_ws(tp_batch_t b, const PriorSweepWs& ws, double* weights, int32_t* status, double* aux) {
    HIP_TRY(b->h, hipSetDevice(b->h->device));
    const size_t n = (size_t)b->W * ws.P * ws.S;
    return download(b->h, {{weights, ws.weights.p, sizeof(double) * n * b->p.k}, {status, ws.status.p, sizeof(int32_t) * n},
                           {aux, ws.aux.p, sizeof(double) * n * TP_AUX_STRIDE}});
}

// ---- window sweeps ---------------------------------------------------------------------------------------------------

// What the two window sweeps share - tp_batch_window_sweep (`tiled` = false, k <= tp_sweep_max_assets()) and
// tp_batch_window_sweep_tiled (above it; `partner`: the sweep below a tiled one, named when k is too small) -: the argument checks, the k range, the drain, the checks against the windows' own row
// counts, the windows per sub-range (L snapshots - conjugate: and C - per window), the sweep's buffers and the copies of the
// caller's arrays - into `ws`, the window sweeps' or the grid sweep's (`sz` given: n_size universes per (window, prior, length),
// w0 per (window, prior, size) and read inside its prefix only, results per (window, prior, length, size); the sizes themselves
// are the caller's to store).  A call refused for its arguments leaves the last sweep's shape and results in place.
// *chunk_out = 0: W = 0, nothing to launch (the sweep's shape is set).
int window_sweep_prepare(tp_batch_t b, WindowSweepWs& ws, const char* name, bool tiled, int32_t n_len, const int32_t* N,
                         const int32_t* rows, const double* delta, int32_t n_prior, const double* n0, const double* w0,
                         int64_t* chunk_out, const SizeAxis* sz = nullptr, const char* partner = "tp_batch_window_sweep") {
    tp_handle_t h = b->h;
    const int k = b->p.k, n_r = b->p.n_r;
    const int64_t W = b->W;
    const bool conj = b->p.strategy == TP_STRATEGY_CONJUGATE;
    *chunk_out = 0;
    if (!b->uploaded) return fail(h, TP_ERR_INVALID, "%s before tp_batch_upload", name);
    if (n_len < 1 || n_len > TP_SWEEP_MAX_RHS)
        return fail(h, TP_ERR_INVALID, "%s: n_len=%d outside [1, %d]", name, n_len, TP_SWEEP_MAX_RHS);
    if (!N) return fail(h, TP_ERR_INVALID, "%s: N is NULL", name);
    for (int l = 0; l < n_len; ++l)
        if (N[l] < 1 || (l > 0 && N[l] <= N[l - 1]))
            return fail(h, TP_ERR_INVALID, "%s: N[%d]=%d: strictly increasing lengths >= 1 expected", name, l, N[l]);
    if (!rows) return fail(h, TP_ERR_INVALID, "%s: rows is NULL", name);
    int rc = sz ? check_size_axis(h, name, *sz, k) : TP_OK;
    if (rc != TP_OK) return rc;
    const int L = n_len;
    const int P = conj ? n_prior : 1;
    const int S = sz ? sz->n_size : 1;
    if (conj) {
        if (n_prior < 1) return fail(h, TP_ERR_INVALID, "%s: n_prior=%d < 1", name, n_prior);
        if (!n0 || !w0) return fail(h, TP_ERR_INVALID, "%s: %s is NULL", name, !n0 ? "n0" : "w0");
        rc = check_finite_sign(h, name, "n0", n0, W * P * L, true);
        if (rc != TP_OK) return rc;
        rc = check_finite_w0(h, name, w0, W * P, k, sz);
        if (rc != TP_OK) return rc;
    } else if (n_prior != 0 || n0 || w0) {
        return fail(h, TP_ERR_INVALID, "%s: a Jeffreys batch takes no priors (n_prior = 0, n0 = w0 = NULL)", name);
    }
    rc = check_sweep_k(h, tiled, name, partner, k);
    if (rc != TP_OK) return rc;
    if (tiled && sz && k + S > tp_max_assets() + 1)
        return fail(h, TP_ERR_UNSUPPORTED, "%s: k=%d with %d sizes exceeds the arena side %d", name, k, S, tp_max_assets() + 1);
    rc = drain_for_sweep(b);
    if (rc != TP_OK) return rc;
    if (W == 0) { ws.P = P; ws.L = L; return TP_OK; }      // (*chunk_out = 0: nothing to launch, the shape is set)
    // the windows' own row counts (the device copy is the one the kernels read), then the checks that need them
    std::vector<int32_t> nw((size_t)W, n_r);
    if (b->n_rows.p) HIP_TRY(h, hipMemcpy(nw.data(), b->n_rows.p, sizeof(int32_t) * (size_t)W, hipMemcpyDeviceToHost));
    for (int64_t w = 0; w < W; ++w)
        for (int l = 0; l < L; ++l) {
            const int32_t r = rows[w * L + l];
            if (r < 1 || r > nw[(size_t)w] || (l > 0 && r < rows[w * L + l - 1]))
                return fail(h, TP_ERR_INVALID, "%s: rows[%lld][%d]=%d: non-decreasing row counts within [1, %d] expected", name,
                            (long long)w, l, r, nw[(size_t)w]);
            if (delta) {
                const double* d = delta + (w * L + l) * (int64_t)n_r;
                for (int i = nw[(size_t)w] - r; i < nw[(size_t)w]; ++i)
                    if (!std::isfinite(d[i]))
                        return fail(h, TP_ERR_INVALID, "%s: delta[%lld][%d][%d] must be finite", name, (long long)w, l, i);
            }
        }
    ws.P = 0; ws.L = 0;                                // every argument check is behind us: a refused call keeps the last results
    const size_t mat_bytes = sizeof(double) * (size_t)k * k;
    const int64_t chunk = sweep_chunk(h, (size_t)(L + (conj ? 1 : 0)) * mat_bytes, (int64_t)P * L, W, true,
                                      tiled ? TP_WINDOW_SWEEP_TILED_WORKSPACE_BYTES : TP_SWEEP_WORKSPACE_BYTES);
    const size_t WL = (size_t)W * (size_t)L, WPL = WL * (size_t)P;
    const size_t WPS = (size_t)W * (size_t)P * (size_t)S, WPLS = WPL * (size_t)S;
    const std::string what = std::string(name) + ": ";
    if (conj) rc = ensure(h, ws.C, mat_bytes * (size_t)chunk, (what + "intraday scatters of one sub-range").c_str());
    if (rc == TP_OK) rc = ensure(h, ws.T, mat_bytes * (size_t)chunk * L, (what + "daily Gram snapshots of one sub-range").c_str());
    if (rc == TP_OK) rc = ensure(h, ws.t, sizeof(double) * WL * k, (what + "daily column sums").c_str());
    if (rc == TP_OK) rc = ensure(h, ws.N, sizeof(int32_t) * (size_t)L, (what + "lengths").c_str());
    if (rc == TP_OK) rc = ensure(h, ws.rows, sizeof(int32_t) * WL, (what + "row counts").c_str());
    if (rc == TP_OK && conj) rc = ensure(h, ws.n0, sizeof(double) * WPL, (what + "prior strengths").c_str());
    if (rc == TP_OK && conj) rc = ensure(h, ws.w0, sizeof(double) * WPS * k, (what + "prior weights").c_str());
    if (rc == TP_OK && delta) rc = ensure(h, ws.delta, sizeof(double) * WL * n_r, (what + "row offsets").c_str());
    if (rc == TP_OK && delta) rc = ensure(h, ws.dv, sizeof(double) * WL * k, (what + "offset-weighted column sums").c_str());
    if (rc == TP_OK && delta) rc = ensure(h, ws.ds, sizeof(double) * WL * 2, (what + "offset sums").c_str());
    if (rc == TP_OK) rc = ensure(h, ws.weights, sizeof(double) * WPLS * k, (what + "weights").c_str());
    if (rc == TP_OK) rc = ensure(h, ws.status, sizeof(int32_t) * WPLS, (what + "statuses").c_str());
    if (rc == TP_OK) rc = ensure(h, ws.aux, sizeof(double) * WPLS * TP_AUX_STRIDE, (what + "aux").c_str());
    if (rc != TP_OK) return rc;
    // the caller's arrays: copied here, no host pointer is kept
    HIP_TRY(h, hipMemcpyAsync(ws.N.p, N, sizeof(int32_t) * (size_t)L, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(ws.rows.p, rows, sizeof(int32_t) * WL, hipMemcpyHostToDevice, h->stream));
    if (conj) {
        HIP_TRY(h, hipMemcpyAsync(ws.n0.p, n0, sizeof(double) * WPL, hipMemcpyHostToDevice, h->stream));
        HIP_TRY(h, hipMemcpyAsync(ws.w0.p, w0, sizeof(double) * WPS * k, hipMemcpyHostToDevice, h->stream));
    }
    if (delta) HIP_TRY(h, hipMemcpyAsync(ws.delta.p, delta, sizeof(double) * WL * n_r, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));       // the copies are done when the call returns, pinned host memory or not
    *chunk_out = chunk;
    return TP_OK;
}

// the segmented Gram's and the delta kernel's arguments over the buffers of `ws`, the same for both window sweeps and the grid sweep
void window_gram_delta_kargs(tp_batch_t b, const WindowSweepWs& ws, int L, tp_window_gram_kargs_t* ga_out, tp_window_delta_kargs_t* da_out) {
    tp_window_gram_kargs_t ga;
    memset(&ga, 0, sizeof ga);
    ga.in = neutral_kargs(b);
    ga.in.w0 = nullptr; ga.in.n0 = nullptr;
    ga.C = b->p.strategy == TP_STRATEGY_CONJUGATE ? (double*)ws.C.p : nullptr;
    ga.T = (double*)ws.T.p; ga.t = (double*)ws.t.p;
    ga.rows = (const int*)ws.rows.p; ga.L = L;
    tp_window_delta_kargs_t da;
    memset(&da, 0, sizeof da);
    da.in = ga.in;
    da.delta = (const double*)ws.delta.p; da.rows = ga.rows;
    da.dv = (double*)ws.dv.p; da.ds = (double*)ws.ds.p; da.L = L;
    *ga_out = ga; *da_out = da;
}

}  // namespace

extern "C" {

// Solve sweep.  Per sub-range the batch's own run kernel stores the matrices of the sub-range (the keep_posterior store) and
// every window's default right-hand side (the keep_rhs store) into the sweep's workspace, then posterior_sweep_kernel solves
// the sub-range's (window, shift) pairs.
int tp_batch_solve_sweep(tp_batch_t b, int32_t n_shift, const double* shift, int32_t n_rhs, const double* rhs,
                         int32_t default_rhs) {
    if (!b) return TP_ERR_INVALID;
    tp_handle_t h = b->h;
    SolveSweepWs& ws = b->sw;
    int S = 0, R = 0;
    int64_t chunk = 0;
    int rc = solve_sweep_prepare(b, "tp_batch_solve_sweep", false, n_shift, shift, n_rhs, rhs, default_rhs, &S, &R, &chunk);
    if (rc != TP_OK || chunk == 0) return rc;
    tp_kargs_t a = neutral_kargs(b);
    a.weights = (double*)ws.weights.p; a.status = (int*)ws.status.p; a.aux = (double*)ws.aux.p;
    a.out_rhs = (double*)ws.rhs0.p;
    a.out_post = (double*)ws.post.p;
    tp_sweep_kargs_t sa;
    memset(&sa, 0, sizeof sa);
    sa.post = (const double*)ws.post.p;
    sa.default_rhs = default_rhs ? (const double*)ws.rhs0.p : nullptr;
    sa.rhs = n_rhs > 0 ? (const double*)ws.rhs.p : nullptr;
    sa.shift = shift ? (const double*)ws.shift.p : nullptr;
    sa.x = (double*)ws.x.p;
    sa.status = (int*)ws.xstatus.p;
    sa.k = b->p.k; sa.S = S; sa.R = R; sa.n_rhs = n_rhs;
    sa.gamma = b->p.gamma;
    return run_sweep(b, chunk, [&](int64_t w0, int64_t n) {
        a.w_first = w0; a.w_count = n;
        a.post_w0 = w0; a.post_count = n;
        const int rcl = launch(b, a, n, false);
        if (rcl != TP_OK) return rcl;
        sa.w_first = w0; sa.w_count = n;
        return launched(h, tp_sweep_launch(sa, h->stream), "sweep kernel");
    }, [&] { ws.S = S; ws.R = R; });
}

// Solve sweep above tp_sweep_max_assets(), on the large-k tiled pipeline.  Per sub-range the batch's own tiled Gram stage - its
// real strategy - leaves M_w in sw.post (the kept-matrix store) and the default right-hand side in sw.rhs0 (the
// kept-right-hand-side store).  Then the sub-range's (window, shift) pairs go through the SWEEP's workspace in groups of its
// capacity: posterior_solve_sweep_tiled.hip fills them, the block steps of the tiled factorisation factorise them and
// forward-substitute the R columns, and the sweep's own kernel back-substitutes.
int tp_batch_solve_sweep_tiled(tp_batch_t b, int32_t n_shift, const double* shift, int32_t n_rhs, const double* rhs,
                               int32_t default_rhs) {
    if (!b) return TP_ERR_INVALID;
    tp_handle_t h = b->h;
    SolveSweepWs& sw = b->sw;
    int S = 0, R = 0;
    int64_t chunk = 0;
    int rc = solve_sweep_prepare(b, "tp_batch_solve_sweep_tiled", true, n_shift, shift, n_rhs, rhs, default_rhs, &S, &R, &chunk);
    if (rc != TP_OK || chunk == 0) return rc;
    // the batch's run workspace as a run would size it, for the Gram stage; the sweep's own for the entries
    tp_tiled_ws_t gws;
    rc = ensure_tiled_ws(b, &gws);
    if (rc != TP_OK) return rc;
    const int64_t gcap = b->tiled_capacity;
    tp_tiled_ws_t ws;
    int64_t cap = 0;
    rc = ensure_sweep_tiled_ws(b, R, chunk * S, &ws, &cap);
    if (rc != TP_OK) return rc;
    tp_kargs_t a = neutral_kargs(b);                   // (the Gram stage writes no weights, statuses or aux)
    a.out_rhs = (double*)sw.rhs0.p;
    a.out_post = (double*)sw.post.p;
    tp_solve_sweep_tiled_kargs_t sa;
    memset(&sa, 0, sizeof sa);
    sa.post = (const double*)sw.post.p;
    sa.default_rhs = default_rhs ? (const double*)sw.rhs0.p : nullptr;
    sa.rhs = n_rhs > 0 ? (const double*)sw.rhs.p : nullptr;
    sa.shift = shift ? (const double*)sw.shift.p : nullptr;
    sa.x = (double*)sw.x.p;
    sa.status = (int*)sw.xstatus.p;
    sa.k = b->p.k; sa.S = S; sa.R = R; sa.n_rhs = n_rhs;
    sa.gamma = b->p.gamma;
    // the block steps read k, w_count (set per group below) and the kernel choices; everything else stays zero
    tp_kargs_t fa;
    memset(&fa, 0, sizeof fa);
    fa.k = b->p.k;
    fa.opts = h->opts;
    return run_sweep(b, chunk, [&](int64_t w0, int64_t n) {
        const int rcg = tiled_gram_stage(b, "tiled solve sweep Gram", {&a}, gws, gcap, w0, n);
        if (rcg != TP_OK) return rcg;
        return in_groups(n * S, cap, [&](int64_t e0, int64_t ne) {
            sa.wc_first = w0;
            sa.e_first = w0 * S + e0; sa.e_count = ne;
            int rce = launched(h, tp_solve_sweep_tiled_fill_launch(sa, ws, h->stream), "tiled solve sweep fill");
            fa.w_count = ne;
            if (rce == TP_OK) rce = launched(h, tp_tiled_block_steps_launch(fa, ws, h->stream), "tiled solve sweep factor");
            if (rce == TP_OK) rce = launched(h, tp_solve_sweep_tiled_solve_launch(sa, ws, h->stream), "tiled solve sweep solve");
            return rce;
        });
    }, [&] { sw.S = S; sw.R = R; });
}

int tp_batch_download_sweep(tp_batch_t b, double* x, int32_t* status) {
    if (!b) return TP_ERR_INVALID;
    tp_handle_t h = b->h;
    const SolveSweepWs& ws = b->sw;
    if (ws.S < 1 || ws.R < 1)
        return fail(h, TP_ERR_INVALID, "tp_batch_download_sweep: no tp_batch_solve_sweep before it");
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t n = (size_t)b->W * ws.S;              // (W = 0: nothing to copy)
    return download(h, {{x, ws.x.p, sizeof(double) * n * ws.R * b->p.k}, {status, ws.xstatus.p, sizeof(int32_t) * n}});
}

int tp_batch_download_sweep_rhs(tp_batch_t b, double* rhs_out) {
    if (!b) return TP_ERR_INVALID;
    tp_handle_t h = b->h;
    if (b->sw.S < 1 || b->sw.R < 1)
        return fail(h, TP_ERR_INVALID, "tp_batch_download_sweep_rhs: no tp_batch_solve_sweep before it");
    HIP_TRY(h, hipSetDevice(h->device));
    if (b->W > 0 && !rhs_out) return fail(h, TP_ERR_INVALID, "tp_batch_download_sweep_rhs: rhs_out is NULL");
    return download(h, {{rhs_out, b->sw.rhs0.p, sizeof(double) * (size_t)b->W * b->p.k}});
}

// Sweep finish (sweep_finish.hip): the Greyserman / Jorion weights from the solutions the last solve sweep of either kind left
// in sw.x.  Every check comes before the drain; the two launches share one timed span and are not awaited.
int tp_batch_sweep_finish(tp_batch_t b, int mode, double gamma, const double* n, const double* kappa, const double* hyper) {
    if (!b) return TP_ERR_INVALID;
    tp_handle_t h = b->h;
    SolveSweepWs& sw = b->sw;
    const char* name = "tp_batch_sweep_finish";
    const int k = b->p.k;
    const int64_t W = b->W;
    if (mode != TP_FINISH_GREYSERMAN && mode != TP_FINISH_JORION) return fail(h, TP_ERR_INVALID, "%s: unknown mode %d", name, mode);
    const bool grey = mode == TP_FINISH_GREYSERMAN;
    if (sw.S < 1 || sw.R < 1) return fail(h, TP_ERR_INVALID, "%s: no tp_batch_solve_sweep before it", name);
    if (sw.R != 2 || !sw.default_rhs)
        return fail(h, TP_ERR_INVALID, "%s: the last sweep solved %d right-hand sides %s the default one: R = 2, the default right-hand side "
                    "and one caller column (the ones vector), is expected", name, sw.R, sw.default_rhs ? "with" : "without");
    if (b->p.gamma != 1.0)
        return fail(h, TP_ERR_INVALID, "%s: the batch's gamma is %g: the sweep has divided its solutions by it already, a batch created "
                    "with gamma = 1 is expected", name, b->p.gamma);
    if (!grey && sw.S != 1)
        return fail(h, TP_ERR_INVALID, "%s: TP_FINISH_JORION takes one shift per window, the last sweep had S=%d", name, sw.S);
    if (!std::isfinite(gamma) || gamma == 0.0) return fail(h, TP_ERR_INVALID, "%s: gamma=%g must be finite and not 0", name, gamma);
    const int S = sw.S;
    const int64_t NG = (S + TP_FINISH_DRAWS_PER_WAVE - 1) / TP_FINISH_DRAWS_PER_WAVE;
    if (k > 64 * TP_FINISH_MAX_SLOTS) return fail(h, TP_ERR_UNSUPPORTED, "%s: k=%d exceeds %d", name, k, 64 * TP_FINISH_MAX_SLOTS);
    if (W > 0x7fffffffLL / NG) return fail(h, TP_ERR_UNSUPPORTED, "%s: W=%lld windows x %lld groups of shifts exceed 2^31", name, (long long)W, (long long)NG);
    if (W > 0) {
        if (!n) return fail(h, TP_ERR_INVALID, "%s: n is NULL", name);
        if (grey && (!kappa || !hyper)) return fail(h, TP_ERR_INVALID, "%s: kappa or hyper is NULL (TP_FINISH_GREYSERMAN)", name);
        for (int64_t w = 0; w < W; ++w) {
            if (!std::isfinite(n[w])) return fail(h, TP_ERR_INVALID, "%s: n[%lld] is not finite", name, (long long)w);
            if (grey && !std::isfinite(kappa[w])) return fail(h, TP_ERR_INVALID, "%s: kappa[%lld] is not finite", name, (long long)w);
        }
        if (grey)
            for (int64_t e = 0; e < W * S; ++e)
                if (!std::isfinite(hyper[2 * e]) || !std::isfinite(hyper[2 * e + 1]))
                    return fail(h, TP_ERR_INVALID, "%s: (xi, eta) of window %lld, shift %lld is not finite", name, (long long)(e / S), (long long)(e % S));
    }
    // ---- device: drain (the sweep ends here; its span is read), upload, two launches that are not awaited
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    int rc = harvest_kernel_time(h);
    if (rc != TP_OK) return rc;
    sw.finished = false;
    sw.finish_stale = false;
    const size_t Wz = (size_t)W;
    rc = ensure(h, sw.fin_n, sizeof(double) * Wz, "tp_batch_sweep_finish: n");
    if (rc == TP_OK && grey) rc = ensure(h, sw.fin_kappa, sizeof(double) * Wz, "tp_batch_sweep_finish: kappa");
    if (rc == TP_OK && grey) rc = ensure(h, sw.fin_hyper, sizeof(double) * 2 * Wz * S, "tp_batch_sweep_finish: (xi, eta)");
    if (rc == TP_OK) rc = ensure(h, sw.fin_part, sizeof(double) * Wz * (size_t)NG * k, "tp_batch_sweep_finish: partial sums");
    if (rc == TP_OK) rc = ensure(h, sw.fin_gstatus, sizeof(int32_t) * Wz * (size_t)NG, "tp_batch_sweep_finish: group statuses");
    if (rc == TP_OK) rc = ensure(h, sw.fin_weights, sizeof(double) * Wz * k, "tp_batch_sweep_finish: weights");
    if (rc == TP_OK) rc = ensure(h, sw.fin_status, sizeof(int32_t) * Wz, "tp_batch_sweep_finish: statuses");
    if (rc == TP_OK) rc = ensure(h, sw.fin_aux, sizeof(double) * 4 * Wz * S, "tp_batch_sweep_finish: aux");
    if (rc != TP_OK) return rc;
    if (W > 0) {
        HIP_TRY(h, hipMemcpyAsync(sw.fin_n.p, n, sizeof(double) * Wz, hipMemcpyHostToDevice, h->stream));
        if (grey) {
            HIP_TRY(h, hipMemcpyAsync(sw.fin_kappa.p, kappa, sizeof(double) * Wz, hipMemcpyHostToDevice, h->stream));
            HIP_TRY(h, hipMemcpyAsync(sw.fin_hyper.p, hyper, sizeof(double) * 2 * Wz * S, hipMemcpyHostToDevice, h->stream));
        }
        HIP_TRY(h, hipStreamSynchronize(h->stream));      // the host arrays are free again
    }
    tp_finish_args_t a;
    memset(&a, 0, sizeof a);
    a.x = (const double*)sw.x.p; a.xstatus = (const int*)sw.xstatus.p; a.t = (const double*)sw.rhs0.p;
    a.n = (const double*)sw.fin_n.p; a.kappa = (const double*)sw.fin_kappa.p; a.hyper = (const double*)sw.fin_hyper.p;
    a.part = (double*)sw.fin_part.p; a.gstatus = (int*)sw.fin_gstatus.p;
    a.weights = (double*)sw.fin_weights.p; a.status = (int*)sw.fin_status.p; a.aux = (double*)sw.fin_aux.p;
    a.gamma = gamma;
    a.W = (int)W; a.S = S; a.k = k; a.mode = grey ? TP_FINISH_KMODE_GREYSERMAN : TP_FINISH_KMODE_JORION;
    const tp_launch_info_t keep_launch = h->last_launch;  // tp_last_launch keeps describing tp_batch_run
    Span& span = timed_span(h);
    HIP_TRY(h, span.begin(h->stream));
    rc = launched(h, tp_finish_launch(a, h->stream), "sweep finish kernel");
    h->last_launch = keep_launch;
    if (rc == TP_OK) rc = timed_done(h, span);
    if (rc != TP_OK) return rc;
    sw.finished = true;
    return TP_OK;
}

int tp_batch_download_sweep_finish(tp_batch_t b, double* weights, int32_t* status, double* aux) {
    if (!b) return TP_ERR_INVALID;
    tp_handle_t h = b->h;
    const SolveSweepWs& sw = b->sw;
    if (!sw.finished)
        return fail(h, TP_ERR_INVALID, sw.finish_stale
                        ? "tp_batch_download_sweep_finish: a solve sweep after the last tp_batch_sweep_finish replaced the solutions it read"
                        : "tp_batch_download_sweep_finish: no tp_batch_sweep_finish before it");
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t W = (size_t)b->W;
    return download(h, {{weights, sw.fin_weights.p, sizeof(double) * W * b->p.k},
                        {status, sw.fin_status.p, sizeof(int32_t) * W},
                        {aux, sw.fin_aux.p, sizeof(double) * 4 * W * sw.S}});
}

// Spectral ridge sweep (posterior_spectral.hip).  Per sub-range the batch's own run kernel stores the matrices of the sub-range
// and every window's t into the spectral workspace (the solve sweep's Gram pass, on buffers of its own), then one
// eigendecomposition per window, the partial sums of every (window, group of draws) in the eigenbasis and the weights.
// Every check comes before the drain: a refused call leaves the last result in place.
int tp_batch_spectral_greyserman(tp_batch_t b, int32_t n_shift, double gamma, const double* n, const double* kappa,
                                 const double* hyper, int32_t keep_vectors) {
    if (!b) return TP_ERR_INVALID;
    tp_handle_t h = b->h;
    SpectralWs& sp = b->sp;
    const char* name = "tp_batch_spectral_greyserman";
    const int k = b->p.k;
    const int64_t W = b->W;
    if (b->p.strategy != TP_STRATEGY_JEFFREYS) return fail(h, TP_ERR_INVALID, "%s applies to the Jeffreys strategy only", name);
    if (!b->uploaded) return fail(h, TP_ERR_INVALID, "%s before tp_batch_upload", name);
    if (b->p.gamma != 1.0)
        return fail(h, TP_ERR_INVALID, "%s: the batch's gamma is %g: a batch created with gamma = 1 is expected (the call takes "
                    "gamma itself)", name, b->p.gamma);
    if (n_shift < 1) return fail(h, TP_ERR_INVALID, "%s: n_shift=%d < 1", name, n_shift);
    if (!std::isfinite(gamma) || gamma == 0.0) return fail(h, TP_ERR_INVALID, "%s: gamma=%g must be finite and not 0", name, gamma);
    const int S = n_shift;
    const int64_t NG = (S + TP_FINISH_DRAWS_PER_WAVE - 1) / TP_FINISH_DRAWS_PER_WAVE;
    if (W > 0) {
        if (!n || !kappa || !hyper) return fail(h, TP_ERR_INVALID, "%s: %s is NULL", name, !n ? "n" : !kappa ? "kappa" : "hyper");
        for (int64_t w = 0; w < W; ++w) {
            if (!std::isfinite(n[w])) return fail(h, TP_ERR_INVALID, "%s: n[%lld] is not finite", name, (long long)w);
            if (!std::isfinite(kappa[w])) return fail(h, TP_ERR_INVALID, "%s: kappa[%lld] is not finite", name, (long long)w);
        }
        for (int64_t e = 0; e < W * S; ++e) {
            if (!std::isfinite(hyper[2 * e]) || !std::isfinite(hyper[2 * e + 1]))
                return fail(h, TP_ERR_INVALID, "%s: (xi, eta) of window %lld, shift %lld is not finite", name, (long long)(e / S), (long long)(e % S));
            if (hyper[2 * e + 1] < 0.0)
                return fail(h, TP_ERR_INVALID, "%s: eta of window %lld, shift %lld is negative", name, (long long)(e / S), (long long)(e % S));
        }
    }
    int rc = check_sweep_k(h, false, name, "", k);
    if (rc != TP_OK) return rc;
    if (W > 0x7fffffffLL / NG) return fail(h, TP_ERR_UNSUPPORTED, "%s: W=%lld windows x %lld groups of shifts exceed 2^31", name, (long long)W, (long long)NG);
    rc = drain_for_sweep(b);
    if (rc != TP_OK) return rc;
    sp.S = 0;
    if (W == 0) { sp.S = S; sp.kept_vectors = keep_vectors != 0; return TP_OK; }
    const size_t mat_bytes = sizeof(double) * (size_t)k * k;
    const size_t Wz = (size_t)W;
    // one sub-range keeps two k x k matrices per window (M and, unless every V is kept, V): the sweeps' workspace rule
    const int64_t chunk = sweep_chunk(h, (keep_vectors ? 1 : 2) * mat_bytes, NG, W, true);
    const std::string what = std::string(name) + ": ";
    rc = ensure(h, sp.post, mat_bytes * (size_t)chunk, (what + "matrices of one sub-range").c_str());
    if (rc == TP_OK) {
        const size_t vbytes = mat_bytes * (keep_vectors ? Wz : (size_t)chunk);
        const std::string vwhat = what + (keep_vectors ? "eigenvectors of all windows, " + std::to_string(vbytes) + " bytes (keep_vectors)"
                                                       : std::string("eigenvectors of one sub-range"));
        rc = ensure(h, sp.V, vbytes, vwhat.c_str());
    }
    if (rc == TP_OK) rc = ensure(h, sp.gw, sizeof(double) * Wz * k, (what + "weights of the Gram pass").c_str());
    if (rc == TP_OK) rc = ensure(h, sp.gs, sizeof(int32_t) * Wz, (what + "statuses of the Gram pass").c_str());
    if (rc == TP_OK) rc = ensure(h, sp.ga, sizeof(double) * Wz * TP_AUX_STRIDE, (what + "aux of the Gram pass").c_str());
    if (rc == TP_OK) rc = ensure(h, sp.t, sizeof(double) * Wz * k, (what + "right-hand sides t").c_str());
    if (rc == TP_OK) rc = ensure(h, sp.lambda, sizeof(double) * Wz * k, (what + "eigenvalues").c_str());
    if (rc == TP_OK) rc = ensure(h, sp.that, sizeof(double) * Wz * k, (what + "rotated t").c_str());
    if (rc == TP_OK) rc = ensure(h, sp.ohat, sizeof(double) * Wz * k, (what + "rotated ones").c_str());
    if (rc == TP_OK) rc = ensure(h, sp.sweeps, sizeof(int32_t) * Wz, (what + "sweep counts").c_str());
    if (rc == TP_OK) rc = ensure(h, sp.jstatus, sizeof(int32_t) * Wz, (what + "eigensolver statuses").c_str());
    if (rc == TP_OK) rc = ensure(h, sp.n, sizeof(double) * Wz, (what + "n").c_str());
    if (rc == TP_OK) rc = ensure(h, sp.kappa, sizeof(double) * Wz, (what + "kappa").c_str());
    if (rc == TP_OK) rc = ensure(h, sp.hyper, sizeof(double) * 2 * Wz * S, (what + "(xi, eta)").c_str());
    if (rc == TP_OK) rc = ensure(h, sp.part, sizeof(double) * Wz * (size_t)NG * k, (what + "partial sums").c_str());
    if (rc == TP_OK) rc = ensure(h, sp.gstatus, sizeof(int32_t) * Wz * (size_t)NG, (what + "group statuses").c_str());
    if (rc == TP_OK) rc = ensure(h, sp.weights, sizeof(double) * Wz * k, (what + "weights").c_str());
    if (rc == TP_OK) rc = ensure(h, sp.status, sizeof(int32_t) * Wz, (what + "statuses").c_str());
    if (rc == TP_OK) rc = ensure(h, sp.aux, sizeof(double) * 4 * Wz * S, (what + "aux").c_str());
    if (rc != TP_OK) return rc;
    // the caller's arrays: copied here, no host pointer is kept
    HIP_TRY(h, hipMemcpyAsync(sp.n.p, n, sizeof(double) * Wz, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(sp.kappa.p, kappa, sizeof(double) * Wz, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(sp.hyper.p, hyper, sizeof(double) * 2 * Wz * S, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));       // the copies are done when the call returns, pinned host memory or not
    tp_kargs_t a = neutral_kargs(b);                   // (no shared block sums: M_w comes from the window's rows alone)
    a.weights = (double*)sp.gw.p; a.status = (int*)sp.gs.p; a.aux = (double*)sp.ga.p;
    a.out_rhs = (double*)sp.t.p;
    a.out_post = (double*)sp.post.p;
    tp_spectral_args_t sa;
    memset(&sa, 0, sizeof sa);
    sa.post = (const double*)sp.post.p; sa.t = (const double*)sp.t.p;
    sa.V = (double*)sp.V.p;
    sa.lambda = (double*)sp.lambda.p; sa.that = (double*)sp.that.p; sa.ohat = (double*)sp.ohat.p;
    sa.sweeps = (int*)sp.sweeps.p; sa.jstatus = (int*)sp.jstatus.p;
    sa.n = (const double*)sp.n.p; sa.kappa = (const double*)sp.kappa.p; sa.hyper = (const double*)sp.hyper.p;
    sa.part = (double*)sp.part.p; sa.gstatus = (int*)sp.gstatus.p;
    sa.weights = (double*)sp.weights.p; sa.status = (int*)sp.status.p; sa.aux = (double*)sp.aux.p;
    sa.gamma = gamma;
    sa.S = S; sa.k = k;
    return run_sweep(b, chunk, [&](int64_t w0, int64_t nw) {
        a.w_first = w0; a.w_count = nw;
        a.post_w0 = w0; a.post_count = nw;
        const int rcl = launch(b, a, nw, false);
        if (rcl != TP_OK) return rcl;
        sa.w_first = w0; sa.w_count = nw; sa.v_first = keep_vectors ? w0 : 0;
        return launched(h, tp_spectral_launch(sa, h->stream), "spectral sweep kernel");
    }, [&] { sp.S = S; sp.kept_vectors = keep_vectors != 0; });
}

int tp_batch_download_spectral(tp_batch_t b, double* weights, int32_t* status, double* aux, double* lambda, int32_t* sweeps,
                               double* V) {
    if (!b) return TP_ERR_INVALID;
    tp_handle_t h = b->h;
    const SpectralWs& sp = b->sp;
    if (sp.S < 1) return fail(h, TP_ERR_INVALID, "tp_batch_download_spectral: no tp_batch_spectral_greyserman before it");
    if (V && !sp.kept_vectors)
        return fail(h, TP_ERR_INVALID, "tp_batch_download_spectral: V asked for, but the last tp_batch_spectral_greyserman had keep_vectors = 0");
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t W = (size_t)b->W, k = (size_t)b->p.k;
    return download(h, {{weights, sp.weights.p, sizeof(double) * W * k},
                        {status, sp.status.p, sizeof(int32_t) * W},
                        {aux, sp.aux.p, sizeof(double) * 4 * W * sp.S},
                        {lambda, sp.lambda.p, sizeof(double) * W * k},
                        {sweeps, sp.sweeps.p, sizeof(int32_t) * W},
                        {V, sp.V.p, sizeof(double) * W * k * k}});
}

// Prior sweep.  Per sub-range the Gram pass stores C and T of the sub-range and t, then posterior_prior_sweep_kernel solves
// the sub-range's (window, prior) pairs.
int tp_batch_prior_sweep(tp_batch_t b, int32_t n_prior, const double* n0, const double* w0) {
    if (!b) return TP_ERR_INVALID;
    tp_handle_t h = b->h;
    PriorSweepWs& ws = b->ps;
    const int P = n_prior;
    int64_t chunk = 0;
    int rc = prior_sweep_prepare(b, ws, "tp_batch_prior_sweep", false, n_prior, n0, w0, &chunk);
    if (rc != TP_OK || chunk == 0) return rc;
    tp_gram_kargs_t ga = gram_pass_kargs(b, ws);
    tp_prior_sweep_kargs_t sa;
    memset(&sa, 0, sizeof sa);
    sa.C = (const double*)ws.C.p; sa.T = (const double*)ws.T.p; sa.t = (const double*)ws.t.p;
    sa.n0 = (const double*)ws.n0.p; sa.w0 = (const double*)ws.w0.p;
    sa.hf_count = (const int*)b->hf_count.p;
    sa.weights = (double*)ws.weights.p; sa.status = (int*)ws.status.p; sa.aux = (double*)ws.aux.p;
    sa.k = b->p.k; sa.P = P; sa.N = b->p.N; sa.m = b->p.m;
    sa.gamma = b->p.gamma;
    return run_sweep(b, chunk, [&](int64_t wf, int64_t n) {
        const int rcg = gram_pass(b, "tp_batch_prior_sweep", "prior sweep Gram", ga, wf, n);
        if (rcg != TP_OK) return rcg;
        sa.w_first = wf; sa.w_count = n;
        return launched(h, tp_prior_sweep_launch(sa, h->stream), "prior sweep kernel");
    }, [&] { ws.P = P; ws.S = 1; });
}

// Prior sweep above tp_sweep_max_assets(), on the large-k tiled pipeline.  Per sub-range the batch's own tiled Gram stage runs
// twice, steered by its arguments - as a Jeffreys batch without centring over the daily rows (T into ps.T through the
// kept-matrix store, t into ps.t through the kept-right-hand-side store) and as a Jeffreys batch centred by the window's row
// count over the INTRADAY rows, the daily-panel fields pointed at the intraday panel (C = Y'Y - (Y'1)(Y'1)'/m into ps.C).
// Then the sub-range's (window, prior) pairs go through the batch's run workspace - borrowed, and grown to hold them - in
// groups of at most tiled_capacity entries: posterior_prior_sweep_tiled.hip fills them, tp_tiled_factor_launch factorises and
// solves them into the sweep's buffers.
int tp_batch_prior_sweep_tiled(tp_batch_t b, int32_t n_prior, const double* n0, const double* w0) {
    if (!b) return TP_ERR_INVALID;
    tp_handle_t h = b->h;
    PriorSweepWs& ps = b->ps;
    const int P = n_prior;
    int64_t chunk = 0;
    int rc = prior_sweep_prepare(b, ps, "tp_batch_prior_sweep_tiled", true, n_prior, n0, w0, &chunk);
    if (rc != TP_OK || chunk == 0) return rc;
    // the batch's own tiled workspace and the pieces of a C w0 per arena entry
    tp_tiled_ws_t ws;
    rc = ensure_tiled_ws(b, &ws, chunk * P);
    if (rc != TP_OK) return rc;
    const int64_t cap = b->tiled_capacity;
    rc = ensure(h, b->t_part, sizeof(double) * (size_t)cap * ws.NS * ws.NS * 64, "tp_batch_prior_sweep_tiled: prior products");
    if (rc != TP_OK) return rc;
    ws.part = (double*)b->t_part.p;

    tp_kargs_t ta, ca;
    tiled_conjugate_gram_kargs(b, ps.T, ps.t, ps.C, &ta, &ca);
    tp_prior_sweep_tiled_kargs_t sa;
    memset(&sa, 0, sizeof sa);
    sa.C = (const double*)ps.C.p; sa.T = (const double*)ps.T.p; sa.t = (const double*)ps.t.p;
    sa.n0 = (const double*)ps.n0.p; sa.w0 = (const double*)ps.w0.p;
    sa.hf_count = (const int*)b->hf_count.p;
    sa.k = b->p.k; sa.P = P; sa.m = b->p.m;
    // factorisation and solve of the arena entries: a conjugate "batch" of (window, prior) pairs writing the sweep's buffers
    tp_kargs_t fa;
    memset(&fa, 0, sizeof fa);
    fa.strategy = TP_STRATEGY_CONJUGATE;
    fa.k = b->p.k; fa.N = b->p.N; fa.n_r = b->p.n_r; fa.m = b->p.m; fa.gamma = b->p.gamma;
    fa.opts = h->opts;
    fa.weights = (double*)ps.weights.p; fa.status = (int*)ps.status.p; fa.aux = (double*)ps.aux.p;
    fa.dbg_w = -1;
    return run_sweep(b, chunk, [&](int64_t wf, int64_t n) {
        const int rcg = tiled_gram_stage(b, "tiled prior sweep Gram", {&ta, &ca}, ws, cap, wf, n);
        if (rcg != TP_OK) return rcg;
        return in_groups(n * P, cap, [&](int64_t e0, int64_t ne) {
            sa.wc_first = wf;
            sa.e_first = wf * P + e0; sa.e_count = ne;
            const int rce = launched(h, tp_prior_sweep_tiled_launch(sa, ws, h->stream), "tiled prior sweep fill");
            if (rce != TP_OK) return rce;
            fa.w_first = sa.e_first; fa.w_count = ne;
            return launched(h, tp_tiled_factor_launch(fa, ws, h->stream), "tiled prior sweep factor");
        });
    }, [&] { ps.P = P; ps.S = 1; });
}

int tp_batch_download_prior_sweep(tp_batch_t b, double* weights, int32_t* status, double* aux) {
    if (!b) return TP_ERR_INVALID;
    if (b->ps.P < 1) return fail(b->h, TP_ERR_INVALID, "tp_batch_download_prior_sweep: no tp_batch_prior_sweep before it");
    return download_prior_ws(b, b->ps, weights, status, aux);
}

// Size sweep.  Sub-ranges as in tp_batch_prior_sweep.  Conjugate: the same Gram pass stores C, T and t.  Jeffreys: the batch's
// own run kernel - as the solve sweep steers it, outputs into the sweep's buffers - keeps M (its centring flag applied) and t;
// it reads the daily inputs only.  Then posterior_size_sweep_kernel factorises every (window, prior) once at k and solves
// every size over its prefix.
int tp_batch_size_sweep(tp_batch_t b, int32_t n_size, const int32_t* sizes, int32_t n_prior, const double* n0, const double* w0) {
    if (!b) return TP_ERR_INVALID;
    tp_handle_t h = b->h;
    PriorSweepWs& ws = b->zs;
    const bool conj = b->p.strategy == TP_STRATEGY_CONJUGATE;
    const int P = conj ? n_prior : 1;
    const SizeAxis sz{n_size, sizes};
    int64_t chunk = 0;
    int rc = prior_sweep_prepare(b, ws, "tp_batch_size_sweep", false, n_prior, n0, w0, &chunk, &sz);
    if (rc != TP_OK || chunk == 0) return rc;
    tp_gram_kargs_t ga = gram_pass_kargs(b, ws);       // conjugate
    tp_kargs_t ja = neutral_kargs(b);                  // Jeffreys
    ja.weights = (double*)ws.gw.p; ja.status = (int*)ws.gs.p; ja.aux = (double*)ws.ga.p;
    ja.out_rhs = (double*)ws.t.p; ja.out_post = (double*)ws.T.p;
    tp_size_sweep_kargs_t sa;
    memset(&sa, 0, sizeof sa);
    sa.C = conj ? (const double*)ws.C.p : nullptr;
    sa.T = (const double*)ws.T.p; sa.t = (const double*)ws.t.p;
    sa.n0 = conj ? (const double*)ws.n0.p : nullptr; sa.w0 = conj ? (const double*)ws.w0.p : nullptr;
    sa.hf_count = (const int*)b->hf_count.p;
    sa.sizes = (const int*)ws.sizes.p;
    sa.weights = (double*)ws.weights.p; sa.status = (int*)ws.status.p; sa.aux = (double*)ws.aux.p;
    sa.k = b->p.k; sa.P = P; sa.S = n_size; sa.N = b->p.N; sa.m = b->p.m;
    sa.gamma = b->p.gamma;
    return run_sweep(b, chunk, [&](int64_t wf, int64_t n) {
        ja.w_first = wf; ja.w_count = n;
        ja.post_w0 = wf; ja.post_count = n;
        const int rcg = conj ? gram_pass(b, "tp_batch_size_sweep", "size sweep Gram", ga, wf, n) : launch(b, ja, n, false);
        if (rcg != TP_OK) return rcg;
        sa.w_first = wf; sa.w_count = n;
        return launched(h, tp_size_sweep_launch(sa, h->stream), "size sweep kernel");
    }, [&] { ws.P = P; ws.S = n_size; });
}

// Size sweep above tp_sweep_max_assets(), on the large-k tiled pipeline.  Per sub-range the batch's own tiled Gram stage stores
// the matrices - conjugate: the two passes of the tiled prior sweep (T, t, raw-moment-centred C); Jeffreys: the batch's real
// strategy and centring flag (M into zs.T, t into zs.t) - through the batch's run workspace, neither grown nor re-shaped.  Then
// the sub-range's (window, prior) pairs go through the SWEEP's workspace (the tiled solve sweep's, at R = n_size) in groups of
// its capacity: posterior_size_sweep_tiled.hip fills them, the block steps factorise them ONCE at k and forward-substitute the
// n_size columns, and the sweep's own kernel back-substitutes every size over its prefix.
int tp_batch_size_sweep_tiled(tp_batch_t b, int32_t n_size, const int32_t* sizes, int32_t n_prior, const double* n0, const double* w0) {
    if (!b) return TP_ERR_INVALID;
    tp_handle_t h = b->h;
    PriorSweepWs& zs = b->zs;
    const bool conj = b->p.strategy == TP_STRATEGY_CONJUGATE;
    const int P = conj ? n_prior : 1;
    const SizeAxis sz{n_size, sizes};
    int64_t chunk = 0;
    int rc = prior_sweep_prepare(b, zs, "tp_batch_size_sweep_tiled", true, n_prior, n0, w0, &chunk, &sz);
    if (rc != TP_OK || chunk == 0) return rc;
    tp_tiled_ws_t gws;
    rc = ensure_tiled_ws(b, &gws);
    if (rc != TP_OK) return rc;
    const int64_t gcap = b->tiled_capacity;
    tp_tiled_ws_t ws;
    int64_t cap = 0;
    rc = ensure_sweep_tiled_ws(b, n_size, chunk * P, &ws, &cap, conj ? tp_size_sweep_tiled_part_doubles(b->p.k, n_size) : 0);
    if (rc != TP_OK) return rc;
    tp_kargs_t ta, ca;                                 // conjugate
    tiled_conjugate_gram_kargs(b, zs.T, zs.t, zs.C, &ta, &ca);
    tp_kargs_t ja = neutral_kargs(b);                  // Jeffreys
    ja.out_rhs = (double*)zs.t.p; ja.out_post = (double*)zs.T.p;
    tp_size_sweep_tiled_kargs_t sa;
    memset(&sa, 0, sizeof sa);
    sa.C = conj ? (const double*)zs.C.p : nullptr;
    sa.T = (const double*)zs.T.p; sa.t = (const double*)zs.t.p;
    sa.n0 = conj ? (const double*)zs.n0.p : nullptr; sa.w0 = conj ? (const double*)zs.w0.p : nullptr;
    sa.hf_count = (const int*)b->hf_count.p;
    sa.sizes = (const int*)zs.sizes.p;
    sa.weights = (double*)zs.weights.p; sa.status = (int*)zs.status.p; sa.aux = (double*)zs.aux.p;
    sa.k = b->p.k; sa.P = P; sa.S = n_size; sa.N = b->p.N; sa.m = b->p.m;
    sa.gamma = b->p.gamma;
    // the block steps read k, w_count (set per group below) and the kernel choices; everything else stays zero
    tp_kargs_t fa;
    memset(&fa, 0, sizeof fa);
    fa.k = b->p.k;
    fa.opts = h->opts;
    return run_sweep(b, chunk, [&](int64_t wf, int64_t n) {
        const int rcg = conj ? tiled_gram_stage(b, "tiled size sweep Gram", {&ta, &ca}, gws, gcap, wf, n)
                             : tiled_gram_stage(b, "tiled size sweep Gram", {&ja}, gws, gcap, wf, n);
        if (rcg != TP_OK) return rcg;
        return in_groups(n * P, cap, [&](int64_t e0, int64_t ne) {
            sa.wc_first = wf;
            sa.e_first = wf * P + e0; sa.e_count = ne;
            int rce = launched(h, tp_size_sweep_tiled_fill_launch(sa, ws, h->stream), "tiled size sweep fill");
            fa.w_count = ne;
            if (rce == TP_OK) rce = launched(h, tp_tiled_block_steps_launch(fa, ws, h->stream), "tiled size sweep factor");
            if (rce == TP_OK) rce = launched(h, tp_size_sweep_tiled_solve_launch(sa, ws, h->stream), "tiled size sweep solve");
            return rce;
        });
    }, [&] { zs.P = P; zs.S = n_size; });
}

int tp_batch_download_size_sweep(tp_batch_t b, double* weights, int32_t* status, double* aux) {
    if (!b) return TP_ERR_INVALID;
    if (b->zs.P < 1 || b->zs.S < 1) return fail(b->h, TP_ERR_INVALID, "tp_batch_download_size_sweep: no tp_batch_size_sweep before it");
    return download_prior_ws(b, b->zs, weights, status, aux);
}

// Window sweep.  Sub-ranges hold L snapshots (conjugate: and C) per window.  Per sub-range the segmented Gram pass
// (posterior_window_gram_nt.hip) stores C once and T_l, t_l after every segment, the delta kernel - with a delta only - forms
// the sums of the rank-two correction, and posterior_window_sweep_kernel solves every (window, prior, length).
int tp_batch_window_sweep(tp_batch_t b, int32_t n_len, const int32_t* N, const int32_t* rows, const double* delta,
                          int32_t n_prior, const double* n0, const double* w0) {
    if (!b) return TP_ERR_INVALID;
    tp_handle_t h = b->h;
    WindowSweepWs& ws = b->wn;
    const char* name = "tp_batch_window_sweep";
    const int k = b->p.k, n_r = b->p.n_r;
    const bool conj = b->p.strategy == TP_STRATEGY_CONJUGATE;
    const int L = n_len;
    const int P = conj ? n_prior : 1;
    int64_t chunk = 0;
    const int rc = window_sweep_prepare(b, ws, name, false, n_len, N, rows, delta, n_prior, n0, w0, &chunk);
    if (rc != TP_OK || chunk == 0) return rc;
    tp_window_gram_kargs_t ga;
    tp_window_delta_kargs_t da;
    window_gram_delta_kargs(b, ws, L, &ga, &da);
    tp_window_sweep_kargs_t sa;
    memset(&sa, 0, sizeof sa);
    sa.C = conj ? (const double*)ws.C.p : nullptr;
    sa.T = (const double*)ws.T.p; sa.t = (const double*)ws.t.p;
    sa.dv = delta ? (const double*)ws.dv.p : nullptr; sa.ds = delta ? (const double*)ws.ds.p : nullptr;
    sa.n0 = conj ? (const double*)ws.n0.p : nullptr; sa.w0 = conj ? (const double*)ws.w0.p : nullptr;
    sa.hf_count = (const int*)b->hf_count.p;
    sa.rows = ga.rows; sa.N = (const int*)ws.N.p;
    sa.weights = (double*)ws.weights.p; sa.status = (int*)ws.status.p; sa.aux = (double*)ws.aux.p;
    sa.k = k; sa.P = P; sa.L = L; sa.m = b->p.m; sa.center_rows = ga.in.center_rows;
    sa.gamma = b->p.gamma;
    return run_sweep(b, chunk, [&](int64_t wf, int64_t n) {
        ga.in.w_first = wf; ga.in.w_count = n;
        const hipError_t e = tp_window_gram_launch(ga, h->stream);
        if (e == hipErrorNotSupported)
            return fail(h, TP_ERR_UNSUPPORTED, "%s: windows of %d daily / %d intraday rows in the index layout are too long "
                                               "for the Gram pass", name, n_r, b->p.m);
        int rcl = launched(h, e, "window sweep Gram");
        if (rcl == TP_OK && delta) {
            da.in.w_first = wf; da.in.w_count = n;
            rcl = launched(h, tp_window_delta_launch(da, h->stream), "window sweep delta kernel");
        }
        if (rcl != TP_OK) return rcl;
        sa.w_first = wf; sa.w_count = n;
        return launched(h, tp_window_sweep_launch(sa, h->stream), "window sweep kernel");
    }, [&] { ws.P = P; ws.L = L; });
}

// Window sweep above tp_sweep_max_assets(), on the large-k tiled pipeline.  Per sub-range: conjugate, the batch's own tiled Gram
// stage over the INTRADAY rows, steered by its arguments as for tp_batch_prior_sweep_tiled, leaves the raw-moment-centred C in
// wn.C (once per window, not once per length); the segmented one-wave Gram (posterior_tiled_window_wave.h) stores the snapshots
// T_l, t_l of every length from ONE pass over the daily rows; the delta kernel - with a delta only - forms the sums of the
// rank-two correction.  Then the sub-range's (window, prior, length) entries go through the batch's run workspace - borrowed,
// and grown to hold them - in groups of ONE length and at most tiled_capacity entries: posterior_window_sweep_tiled.hip fills
// them, tp_tiled_factor_launch factorises and solves them with N = N[l] into staging rows, and the scatter kernel puts those
// into the sweep's result slots.
int tp_batch_window_sweep_tiled(tp_batch_t b, int32_t n_len, const int32_t* N, const int32_t* rows, const double* delta,
                                int32_t n_prior, const double* n0, const double* w0) {
    if (!b) return TP_ERR_INVALID;
    tp_handle_t h = b->h;
    WindowSweepWs& wn = b->wn;
    const char* name = "tp_batch_window_sweep_tiled";
    const int k = b->p.k;
    const bool conj = b->p.strategy == TP_STRATEGY_CONJUGATE;
    const int L = n_len;
    const int P = conj ? n_prior : 1;
    int64_t chunk = 0;
    int rc = window_sweep_prepare(b, wn, name, true, n_len, N, rows, delta, n_prior, n0, w0, &chunk);
    if (rc != TP_OK || chunk == 0) return rc;
    // the batch's own tiled workspace: the Gram stage of C, then the entries; staging rows for one group of entries
    tp_tiled_ws_t ws;
    rc = ensure_tiled_ws(b, &ws, chunk * P);
    if (rc != TP_OK) return rc;
    const int64_t cap = b->tiled_capacity;
    const int64_t gmax = std::min<int64_t>(cap, chunk * P);
    const std::string what = std::string(name) + ": ";
    rc = ensure(h, wn.stage_w, sizeof(double) * (size_t)gmax * k, (what + "weights of one group of entries").c_str());
    if (rc == TP_OK) rc = ensure(h, wn.stage_s, sizeof(int32_t) * (size_t)gmax, (what + "statuses of one group of entries").c_str());
    if (rc == TP_OK) rc = ensure(h, wn.stage_a, sizeof(double) * (size_t)gmax * TP_AUX_STRIDE, (what + "aux of one group of entries").c_str());
    if (rc == TP_OK && conj) rc = ensure(h, wn.cw, sizeof(double) * (size_t)chunk * P * k, (what + "prior products of one sub-range").c_str());
    if (rc == TP_OK && conj) rc = ensure(h, wn.cq, sizeof(double) * (size_t)chunk * P, (what + "prior quadratic forms of one sub-range").c_str());
    if (rc != TP_OK) return rc;

    tp_kargs_t ta, ca;                                 // conjugate: `ca`, the pass over the intraday rows, alone (T_l, t_l: the segmented Gram)
    tiled_conjugate_gram_kargs(b, wn.T, wn.t, wn.C, &ta, &ca);
    (void)ta;
    tp_window_gram_kargs_t ga;
    tp_window_delta_kargs_t da;
    window_gram_delta_kargs(b, wn, L, &ga, &da);
    tp_window_sweep_tiled_kargs_t sa;
    memset(&sa, 0, sizeof sa);
    sa.C = conj ? (const double*)wn.C.p : nullptr;
    sa.T = (const double*)wn.T.p; sa.t = (const double*)wn.t.p;
    sa.dv = delta ? (const double*)wn.dv.p : nullptr; sa.ds = delta ? (const double*)wn.ds.p : nullptr;
    sa.n0 = conj ? (const double*)wn.n0.p : nullptr; sa.w0 = conj ? (const double*)wn.w0.p : nullptr;
    sa.hf_count = (const int*)b->hf_count.p;
    sa.rows = ga.rows;
    sa.cw = (double*)wn.cw.p; sa.cq = (double*)wn.cq.p;
    sa.stage_w = (const double*)wn.stage_w.p; sa.stage_s = (const int*)wn.stage_s.p; sa.stage_a = (const double*)wn.stage_a.p;
    sa.weights = (double*)wn.weights.p; sa.status = (int*)wn.status.p; sa.aux = (double*)wn.aux.p;
    sa.k = k; sa.P = P; sa.L = L; sa.m = b->p.m; sa.center_rows = ga.in.center_rows;
    // factorisation and solve of one group of entries: a "batch" of (window, prior) pairs at ONE length, N = N[l], writing the
    // staging rows (entry e -> row e); n0 travels through ws.scal
    tp_kargs_t fa;
    memset(&fa, 0, sizeof fa);
    fa.strategy = b->p.strategy;
    fa.k = k; fa.n_r = b->p.n_r; fa.m = b->p.m; fa.gamma = b->p.gamma;
    fa.opts = h->opts;
    fa.weights = (double*)wn.stage_w.p; fa.status = (int*)wn.stage_s.p; fa.aux = (double*)wn.stage_a.p;
    fa.dbg_w = -1;
    return run_sweep(b, chunk, [&](int64_t wf, int64_t n) {
        int rcg = conj ? tiled_gram_stage(b, "tiled window sweep Gram", {&ca}, ws, cap, wf, n) : TP_OK;
        if (rcg != TP_OK) return rcg;
        ga.in.w_first = wf; ga.in.w_count = n;
        rcg = launched(h, tp_tiled_window_gram_launch(ga, h->stream), "tiled window sweep segmented Gram");
        if (rcg == TP_OK && delta) {
            da.in.w_first = wf; da.in.w_count = n;
            rcg = launched(h, tp_window_delta_launch(da, h->stream), "window sweep delta kernel");
        }
        if (rcg != TP_OK) return rcg;
        sa.wc_first = wf;
        if (conj) {
            sa.l = 0; sa.wp_first = wf * P; sa.e_count = n * P;
            rcg = launched(h, tp_window_sweep_tiled_cw_launch(sa, h->stream), "tiled window sweep prior products");
            if (rcg != TP_OK) return rcg;
        }
        for (int l = 0; l < L; ++l) {
            sa.l = l; sa.N = N[l];
            fa.N = N[l];
            const int rcl = in_groups(n * P, cap, [&](int64_t e0, int64_t ne) {
                sa.wp_first = wf * P + e0; sa.e_count = ne;
                int rce = launched(h, tp_window_sweep_tiled_fill_launch(sa, ws, h->stream), "tiled window sweep fill");
                fa.w_first = 0; fa.w_count = ne;
                if (rce == TP_OK) rce = launched(h, tp_tiled_factor_launch(fa, ws, h->stream), "tiled window sweep factor");
                if (rce == TP_OK) rce = launched(h, tp_window_sweep_tiled_scatter_launch(sa, h->stream), "tiled window sweep scatter");
                return rce;
            });
            if (rcl != TP_OK) return rcl;
        }
        return TP_OK;
    }, [&] { wn.P = P; wn.L = L; });
}

int tp_batch_download_window_sweep(tp_batch_t b, double* weights, int32_t* status, double* aux) {
    if (!b) return TP_ERR_INVALID;
    tp_handle_t h = b->h;
    const WindowSweepWs& ws = b->wn;
    if (ws.P < 1 || ws.L < 1) return fail(h, TP_ERR_INVALID, "tp_batch_download_window_sweep: no tp_batch_window_sweep before it");
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t n = (size_t)b->W * ws.P * ws.L;
    return download(h, {{weights, ws.weights.p, sizeof(double) * n * b->p.k}, {status, ws.status.p, sizeof(int32_t) * n},
                        {aux, ws.aux.p, sizeof(double) * n * TP_AUX_STRIDE}});
}

// Grid sweep.  The window sweep's sub-ranges and Gram stages - the segmented Gram pass stores C once and (T_l, t_l) per length at
// the batch's k, the delta kernel forms the sums of the rank-two correction - into the grid sweep's own workspace; then
// posterior_grid_sweep_kernel factorises every (window, prior, length) once at k and solves every size over its prefix.
int tp_batch_grid_sweep(tp_batch_t b, int32_t n_size, const int32_t* sizes, int32_t n_len, const int32_t* N, const int32_t* rows,
                        const double* delta, int32_t n_prior, const double* n0, const double* w0) {
    if (!b) return TP_ERR_INVALID;
    tp_handle_t h = b->h;
    GridSweepWs& ws = b->gr;
    const char* name = "tp_batch_grid_sweep";
    const int k = b->p.k, n_r = b->p.n_r;
    const bool conj = b->p.strategy == TP_STRATEGY_CONJUGATE;
    const int L = n_len, S = n_size;
    const int P = conj ? n_prior : 1;
    const SizeAxis sz{n_size, sizes};
    int64_t chunk = 0;
    int rc = window_sweep_prepare(b, ws, name, false, n_len, N, rows, delta, n_prior, n0, w0, &chunk, &sz);
    if (rc != TP_OK) return rc;
    if (chunk == 0) { ws.S = S; return TP_OK; }            // W = 0: nothing to launch, the shape is set
    ws.S = 0;
    rc = ensure(h, ws.sizes, sizeof(int32_t) * (size_t)S, "tp_batch_grid_sweep: sizes");
    if (rc != TP_OK) return rc;
    HIP_TRY(h, hipMemcpyAsync(ws.sizes.p, sizes, sizeof(int32_t) * (size_t)S, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    tp_window_gram_kargs_t ga;
    tp_window_delta_kargs_t da;
    window_gram_delta_kargs(b, ws, L, &ga, &da);
    tp_grid_sweep_kargs_t sa;
    memset(&sa, 0, sizeof sa);
    sa.C = conj ? (const double*)ws.C.p : nullptr;
    sa.T = (const double*)ws.T.p; sa.t = (const double*)ws.t.p;
    sa.dv = delta ? (const double*)ws.dv.p : nullptr; sa.ds = delta ? (const double*)ws.ds.p : nullptr;
    sa.n0 = conj ? (const double*)ws.n0.p : nullptr; sa.w0 = conj ? (const double*)ws.w0.p : nullptr;
    sa.hf_count = (const int*)b->hf_count.p;
    sa.rows = ga.rows; sa.N = (const int*)ws.N.p; sa.sizes = (const int*)ws.sizes.p;
    sa.weights = (double*)ws.weights.p; sa.status = (int*)ws.status.p; sa.aux = (double*)ws.aux.p;
    sa.k = k; sa.P = P; sa.L = L; sa.S = S; sa.m = b->p.m; sa.center_rows = ga.in.center_rows;
    sa.gamma = b->p.gamma;
    return run_sweep(b, chunk, [&](int64_t wf, int64_t n) {
        ga.in.w_first = wf; ga.in.w_count = n;
        const hipError_t e = tp_window_gram_launch(ga, h->stream);
        if (e == hipErrorNotSupported)
            return fail(h, TP_ERR_UNSUPPORTED, "%s: windows of %d daily / %d intraday rows in the index layout are too long "
                                               "for the Gram pass", name, n_r, b->p.m);
        int rcl = launched(h, e, "grid sweep Gram");
        if (rcl == TP_OK && delta) {
            da.in.w_first = wf; da.in.w_count = n;
            rcl = launched(h, tp_window_delta_launch(da, h->stream), "grid sweep delta kernel");
        }
        if (rcl != TP_OK) return rcl;
        sa.w_first = wf; sa.w_count = n;
        return launched(h, tp_grid_sweep_launch(sa, h->stream), "grid sweep kernel");
    }, [&] { ws.P = P; ws.L = L; ws.S = S; });
}

// Grid sweep above tp_sweep_max_assets(), on the large-k tiled pipeline: the tiled window sweep's Gram stages into the grid
// sweep's workspace, the tiled size sweep's entries.  Per sub-range (the tiled window sweep's rule and budget): conjugate, the
// batch's own tiled Gram stage over the INTRADAY rows leaves the raw-moment-centred C in gr.C through the batch's run workspace,
// neither grown nor re-shaped; the segmented one-wave Gram stores the snapshots T_l, t_l at the batch's k; the delta kernel - with
// a delta only - forms the sums of the rank-two correction; one kernel forms the S truncated prior products per (window, prior).
// Then the sub-range's (window, prior, length) entries go through the SWEEP's workspace (the tiled solve sweep's, at R = n_size)
// in groups of its capacity, ALL lengths together: posterior_grid_sweep_tiled.hip fills them, the block steps factorise them ONCE
// at k and forward-substitute the n_size columns, and the sweep's own kernel - which reads N and n0 per entry - back-substitutes
// every size over its prefix and writes the results to their slots.
int tp_batch_grid_sweep_tiled(tp_batch_t b, int32_t n_size, const int32_t* sizes, int32_t n_len, const int32_t* N, const int32_t* rows,
                              const double* delta, int32_t n_prior, const double* n0, const double* w0) {
    if (!b) return TP_ERR_INVALID;
    tp_handle_t h = b->h;
    GridSweepWs& gr = b->gr;
    const char* name = "tp_batch_grid_sweep_tiled";
    const int k = b->p.k;
    const bool conj = b->p.strategy == TP_STRATEGY_CONJUGATE;
    const int L = n_len, S = n_size;
    const int P = conj ? n_prior : 1;
    const SizeAxis sz{n_size, sizes};
    int64_t chunk = 0;
    int rc = window_sweep_prepare(b, gr, name, true, n_len, N, rows, delta, n_prior, n0, w0, &chunk, &sz, "tp_batch_grid_sweep");
    if (rc != TP_OK) return rc;
    if (chunk == 0) { gr.S = S; return TP_OK; }            // W = 0: nothing to launch, the shape is set
    gr.S = 0;
    // the batch's run workspace as a run would size it, for the pass over the intraday rows; the sweep's own for the entries
    tp_tiled_ws_t gws;
    memset(&gws, 0, sizeof gws);
    int64_t gcap = 0;
    if (conj) {
        rc = ensure_tiled_ws(b, &gws);
        if (rc != TP_OK) return rc;
        gcap = b->tiled_capacity;
    }
    tp_tiled_ws_t ws;
    int64_t cap = 0;
    rc = ensure_sweep_tiled_ws(b, S, chunk * P * L, &ws, &cap);
    if (rc != TP_OK) return rc;
    const std::string what = std::string(name) + ": ";
    rc = ensure(h, gr.sizes, sizeof(int32_t) * (size_t)S, (what + "sizes").c_str());
    if (rc == TP_OK) rc = ensure(h, gr.mdiag, sizeof(double) * (size_t)cap * k, (what + "diagonals of one group of entries").c_str());
    if (rc == TP_OK && conj) rc = ensure(h, gr.cw, sizeof(double) * (size_t)chunk * P * S * k, (what + "prior products of one sub-range").c_str());
    if (rc == TP_OK && conj) rc = ensure(h, gr.cq, sizeof(double) * (size_t)chunk * P * S, (what + "prior quadratic forms of one sub-range").c_str());
    if (rc != TP_OK) return rc;
    HIP_TRY(h, hipMemcpyAsync(gr.sizes.p, sizes, sizeof(int32_t) * (size_t)S, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));

    tp_kargs_t ta, ca;                                 // conjugate: `ca`, the pass over the intraday rows, alone (T_l, t_l: the segmented Gram)
    tiled_conjugate_gram_kargs(b, gr.T, gr.t, gr.C, &ta, &ca);
    (void)ta;
    tp_window_gram_kargs_t ga;
    tp_window_delta_kargs_t da;
    window_gram_delta_kargs(b, gr, L, &ga, &da);
    tp_grid_sweep_tiled_kargs_t sa;
    memset(&sa, 0, sizeof sa);
    sa.C = conj ? (const double*)gr.C.p : nullptr;
    sa.T = (const double*)gr.T.p; sa.t = (const double*)gr.t.p;
    sa.dv = delta ? (const double*)gr.dv.p : nullptr; sa.ds = delta ? (const double*)gr.ds.p : nullptr;
    sa.n0 = conj ? (const double*)gr.n0.p : nullptr; sa.w0 = conj ? (const double*)gr.w0.p : nullptr;
    sa.hf_count = (const int*)b->hf_count.p;
    sa.rows = ga.rows; sa.N = (const int*)gr.N.p; sa.sizes = (const int*)gr.sizes.p;
    sa.cv = conj ? (double*)gr.cw.p : nullptr; sa.cq = conj ? (double*)gr.cq.p : nullptr;
    sa.mdiag = (double*)gr.mdiag.p;
    sa.weights = (double*)gr.weights.p; sa.status = (int*)gr.status.p; sa.aux = (double*)gr.aux.p;
    sa.k = k; sa.P = P; sa.L = L; sa.S = S; sa.m = b->p.m; sa.center_rows = ga.in.center_rows;
    sa.gamma = b->p.gamma;
    // the block steps read k, w_count (set per group below) and the kernel choices; everything else stays zero
    tp_kargs_t fa;
    memset(&fa, 0, sizeof fa);
    fa.k = k;
    fa.opts = h->opts;
    return run_sweep(b, chunk, [&](int64_t wf, int64_t n) {
        int rcg = conj ? tiled_gram_stage(b, "tiled grid sweep Gram", {&ca}, gws, gcap, wf, n) : TP_OK;
        if (rcg != TP_OK) return rcg;
        ga.in.w_first = wf; ga.in.w_count = n;
        rcg = launched(h, tp_tiled_window_gram_launch(ga, h->stream), "tiled grid sweep segmented Gram");
        if (rcg == TP_OK && delta) {
            da.in.w_first = wf; da.in.w_count = n;
            rcg = launched(h, tp_window_delta_launch(da, h->stream), "grid sweep delta kernel");
        }
        if (rcg != TP_OK) return rcg;
        sa.wc_first = wf;
        if (conj) {
            sa.wp_first = wf * P; sa.wp_count = n * P;
            rcg = launched(h, tp_grid_sweep_tiled_cw_launch(sa, h->stream), "tiled grid sweep prior products");
            if (rcg != TP_OK) return rcg;
        }
        return in_groups(n * P * L, cap, [&](int64_t e0, int64_t ne) {
            sa.e_first = wf * P * L + e0; sa.e_count = ne;
            int rce = launched(h, tp_grid_sweep_tiled_fill_launch(sa, ws, h->stream), "tiled grid sweep fill");
            fa.w_count = ne;
            if (rce == TP_OK) rce = launched(h, tp_tiled_block_steps_launch(fa, ws, h->stream), "tiled grid sweep factor");
            if (rce == TP_OK) rce = launched(h, tp_grid_sweep_tiled_solve_launch(sa, ws, h->stream), "tiled grid sweep solve");
            return rce;
        });
    }, [&] { gr.P = P; gr.L = L; gr.S = S; });
}

int tp_batch_download_grid_sweep(tp_batch_t b, double* weights, int32_t* status, double* aux) {
    if (!b) return TP_ERR_INVALID;
    tp_handle_t h = b->h;
    const GridSweepWs& ws = b->gr;
    if (ws.P < 1 || ws.L < 1 || ws.S < 1) return fail(h, TP_ERR_INVALID, "tp_batch_download_grid_sweep: no tp_batch_grid_sweep before it");
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t n = (size_t)b->W * ws.P * ws.L * ws.S;
    return download(h, {{weights, ws.weights.p, sizeof(double) * n * b->p.k}, {status, ws.status.p, sizeof(int32_t) * n},
                        {aux, ws.aux.p, sizeof(double) * n * TP_AUX_STRIDE}});
}

}  // extern "C"
