// tangency_api.cpp - C-ABI of libtangency.so (include/tangency_posterior.h): lifetime, uploads, runs, downloads, timing
// and regions (the sweeps: tangency_sweep.cpp, the gather: tangency_comm.cpp).  Compiled with hipcc; no kernels in this file.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <atomic>
#include <memory>
#include <mutex>
#include <new>

#include "tangency_host.h"

using namespace tp_host;

static_assert(TP_STATUS_NOT_PD == TP_KSTATUS_NOT_PD && TP_STATUS_NONFINITE == TP_KSTATUS_NONFINITE &&
              TP_STATUS_BAD_DENOM == TP_KSTATUS_BAD_DENOM, "status codes out of sync");
static_assert(TP_UNIQUE_ID_BYTES == NCCL_UNIQUE_ID_BYTES, "unique id size");

namespace { thread_local std::string g_create_error; }   // tp_last_error(NULL): why tp_create failed

int tp_host::fail(tp_handle_t h, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (h) h->err = buf; else g_create_error = buf;
    return code;
}

int tp_host::ensure(tp_handle_t h, DevBuf& b, size_t bytes, const char* what) {
    if (bytes == 0) bytes = 8;
    const hipError_t e = b.reserve(bytes);
    if (e != hipSuccess) return fail(h, TP_ERR_HIP, "cannot allocate %zu bytes (%s): %s", bytes, what, hipGetErrorString(e));
    return TP_OK;
}

int tp_host::download(tp_handle_t h, std::initializer_list<Copy> copies) {
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    int rc = harvest_kernel_time(h);
    if (rc != TP_OK) return rc;
    for (const Copy& c : copies)
        if (c.dst && c.bytes) HIP_TRY(h, hipMemcpyAsync(c.dst, c.src, c.bytes, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return TP_OK;
}

namespace {

// ---- lifetime ---------------------------------------------------------------------------------------------------
// Every live handle is registered here.  A C atexit handler - registered by the first tp_create, i.e. AFTER the HIP and
// RCCL libraries registered their own static teardown, so it runs BEFORE them - destroys what the caller left alive
// (batches first, then the RCCL communicator, streams, events) while the runtimes still work, and then marks the
// library as shut down: a tp_destroy / tp_batch_destroy that arrives later (an object finalised by a host language
// during its own exit) frees nothing on the device and makes no HIP / RCCL call.  Round 2's exit-time aborts
// (std::bad_variant_access, a core dump after a failed test) were exactly such calls and leaked communicators.
std::mutex g_registry_mutex;
std::vector<tp_handle_t> g_live_handles;
std::atomic<bool> g_shut_down{false};
std::atomic<bool> g_exiting{false};        // inside the exit handler: release resources, never start a collective
bool g_atexit_registered = false;

bool runtime_gone(hipError_t e) {
    return e == hipErrorDeinitialized || e == hipErrorNotInitialized || e == hipErrorContextIsDestroyed ||
           e == hipErrorInvalidContext;
}

int env_int(const char* name, int dflt) {
    const char* e = getenv(name);
    return (e && *e) ? atoi(e) : dflt;
}

int destroy_handle(tp_handle_t h, bool device_calls);
int destroy_batch(tp_batch_t b, bool device_calls);

void shutdown_at_exit() {
    g_exiting.store(true);
    std::vector<tp_handle_t> live;
    { std::lock_guard<std::mutex> lk(g_registry_mutex); live.swap(g_live_handles); }
    for (tp_handle_t h : live) (void)destroy_handle(h, true);
    g_shut_down.store(true);
}

int put(tp_handle_t h, DevBuf& b, const void* src, size_t bytes, const char* what, hipStream_t st = nullptr) {
    if (!src) { b.release(); return TP_OK; }   // optional input absent: drop any stale copy
    int rc = ensure(h, b, bytes, what);
    if (rc != TP_OK) return rc;
    HIP_TRY(h, hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, st ? st : h->stream));
    return TP_OK;
}

int check_params(tp_handle_t h, const tp_params_t* p, int64_t W) {
    if (!p) return fail(h, TP_ERR_INVALID, "params is NULL");
    if (W < 0) return fail(h, TP_ERR_INVALID, "W=%lld < 0", (long long)W);
    if (p->k < 1) return fail(h, TP_ERR_INVALID, "k=%d < 1", p->k);
    if (p->N < 1 || p->n_r < 1) return fail(h, TP_ERR_INVALID, "N=%d n_r=%d must be >= 1", p->N, p->n_r);
    if (p->strategy != TP_STRATEGY_CONJUGATE && p->strategy != TP_STRATEGY_JEFFREYS)
        return fail(h, TP_ERR_INVALID, "unknown strategy %d", p->strategy);
    if (p->strategy == TP_STRATEGY_CONJUGATE && p->m < 2)
        return fail(h, TP_ERR_INVALID, "conjugate prior needs m >= 2 intraday returns (m=%d)", p->m);
    if (!(p->gamma > 0.0) && !(p->gamma < 0.0)) return fail(h, TP_ERR_INVALID, "gamma must be non-zero");
    if (p->k > tp_max_assets())
        return fail(h, TP_ERR_UNSUPPORTED, "k=%d exceeds the largest supported universe %d", p->k, tp_max_assets());
    return TP_OK;
}

}  // namespace

tp_kargs_t tp_host::make_kargs(tp_batch_t b) {
    tp_kargs_t a;
    memset(&a, 0, sizeof a);
    a.panel = (const double*)b->panel.p;
    a.start = (const long long*)b->start.p;
    a.row_idx = (const int*)b->row_idx.p;
    a.n_rows = (const int*)b->n_rows.p;
    a.col_idx = (const int*)b->col_idx.p;
    a.rf_adj = (const double*)b->rf_adj.p;
    a.hf_panel = (const double*)b->hf_panel.p;
    a.hf_start = (const long long*)b->hf_start.p;
    a.hf_row_idx = (const int*)b->hf_row_idx.p;
    a.hf_count = (const int*)b->hf_count.p;
    a.w0 = (const double*)b->w0.p;
    a.n0 = (const double*)b->n0.p;
    a.prefix = (b->prefix_nblk > 0 && !b->prefix_per_sub) ? (const double*)b->prefix.p : nullptr;
    a.prefix_nblk = b->prefix_per_sub ? 0 : b->prefix_nblk;
    a.prefix_blk0 = 0;
    a.winsum = nullptr;
    for (int i = 0; i < 4; ++i) a.winsum_L[i] = 0;
    if (b->prefix_nblk > 0 && !b->prefix_per_sub) {      // block Grams first, the block-window tables behind them
        const size_t slot = b->p.k <= tp_fused_max_assets() ? tp_fused_slot_doubles(b->p.k) : tp_tiled_slot_doubles(b->p.k);
        a.winsum = (const double*)b->prefix.p + (size_t)b->prefix_nblk * slot;
        for (int i = 0; i < 4; ++i) a.winsum_L[i] = b->winsum_L[i];
        if (b->winsum_zero) {                            // the all-zero slot behind the last table (plan_shared_gram)
            int n_L = 0;
            while (n_L < TP_WINSUM_MAX_L && b->winsum_L[n_L] > 0) ++n_L;
            a.winsum_zero = a.winsum + (size_t)n_L * (size_t)b->prefix_nblk * slot;
        }
    }
    a.rhs = (const double*)b->rhs.p;
    a.shift = (const double*)b->shift.p;
    a.center_rows = (b->p.flags & TP_FLAG_NO_CENTER) ? 2 : (b->p.flags & TP_FLAG_CENTER_BY_ROWS) ? 1 : 0;
    a.phase_limit = 0;
#ifdef TP_STAMP
    a.phase_limit = b->h->phase_limit;                // diagnostic build only (TP_PHASE_LIMIT, read in tp_create)
#endif
    a.opts = b->h->opts;
    a.shared_tables = b->h->shared_tables;
    a.weights = b->out_weights();
    a.status = (int*)b->out_status();
    a.aux = (double*)b->aux.p;
    a.out_rhs = (double*)b->out_rhs.p;
    a.out_post = (double*)b->post.p;
    a.post_w0 = b->post_w0;
    a.post_count = b->post.p ? b->post_count : 0;
    a.stamps = (long long*)b->stamps.p;
    a.dbg_S1 = nullptr;
    a.dbg_w = -1;
    a.w_first = 0;
    a.w_count = b->W;
    a.panel_ld = b->panel_ld;
    a.hf_ld = b->hf_ld;
    (void)tp_batch_addressing(b, &a.panel_off32, &a.hf_off32);   // tp_addressing_flags of the two panels: 32-bit offsets or not
    a.k = b->p.k; a.N = b->p.N; a.n_r = b->p.n_r; a.m = b->p.m; a.strategy = b->p.strategy;
    a.gamma = b->p.gamma;
    return a;
}

Span& tp_host::timed_span(tp_handle_t h) {
    return h->in_region && h->ring_used < (int)h->ring.size() ? h->ring[(size_t)h->ring_used] : h->kernel_span;
}

int tp_host::timed_done(tp_handle_t h, Span& span) {
    HIP_TRY(h, span.end(h->stream));
    if (&span != &h->kernel_span) ++h->ring_used;
    return TP_OK;
}

int tp_host::launch(tp_batch_t b, const tp_kargs_t& a, int64_t count, bool timed) {
    tp_handle_t h = b->h;
    if (count <= 0) return TP_OK;
    if (count > 0x7fffffffLL) return fail(h, TP_ERR_INVALID, "too many windows in one launch");
    Span* span = timed ? &timed_span(h) : nullptr;
    if (a.k <= tp_fused_max_assets()) {
        if (span) HIP_TRY(h, span->begin(h->stream));
        hipError_t e = tp_fused_launch(a, (int)count, h->stream, &h->last_launch, nullptr);
        if (e != hipSuccess) return fail(h, TP_ERR_HIP, "kernel launch failed: %s", hipGetErrorString(e));
        return span ? timed_done(h, *span) : TP_OK;
    }
    // large-k path: sub-batches of in-flight windows through the tiled pipeline
    if (a.dbg_S1 != nullptr) return fail(h, TP_ERR_UNSUPPORTED, "matrix read-back is not available on the large-k path");
    tp_tiled_ws_t ws;
    int rc = ensure_tiled_ws(b, &ws);
    if (rc != TP_OK) return rc;
    if (span) HIP_TRY(h, span->begin(h->stream));
    for (int64_t w0 = 0; w0 < count; w0 += b->tiled_capacity) {
        tp_kargs_t sub = a;
        sub.w_first = a.w_first + w0;
        sub.w_count = (count - w0 < b->tiled_capacity) ? (count - w0) : b->tiled_capacity;
        if (b->prefix_per_sub) {
            rc = plan_daily_tables(b, sub);
            if (rc != TP_OK) return rc;
        }
        if (b->hf_B > 0 && a.strategy == TP_STRATEGY_CONJUGATE) {
            rc = plan_hf_tables(b, sub);
            if (rc != TP_OK) return rc;
        }
        // (per-sub-batch tables: every sub-batch builds its own; a whole-panel table: the first one builds it)
        hipError_t e = tp_tiled_launch(sub, ws, h->stream, b->prefix_per_sub || w0 == 0);
        if (e != hipSuccess) return fail(h, TP_ERR_HIP, "tiled pipeline launch failed: %s", hipGetErrorString(e));
    }
    h->last_launch = tp_launch_info_t{(int)(count < b->tiled_capacity ? count : b->tiled_capacity), 256, 36864, ws.NS * 4};
    return span ? timed_done(h, *span) : TP_OK;
}

// Before and after the launches of a tp_batch_run or a sweep.
int tp_host::begin_launches(tp_batch_t b) {
    tp_handle_t h = b->h;
    HIP_TRY(h, hipSetDevice(h->device));
    if (b->upload_pending) {          // tp_batch_upload_async: the kernel stream waits for the copy stream's event
        HIP_TRY(h, hipStreamWaitEvent(h->stream, b->upload_done, 0));
        b->upload_pending = false;
    }
    return TP_OK;
}

int tp_host::end_launches(tp_batch_t b) {
    tp_handle_t h = b->h;
    // the end of the launches, recorded EVERY time: a later tp_batch_upload_async of this batch - also the first one,
    // after synchronous uploads - makes the copy stream wait for it before it overwrites what the launches read
    HIP_TRY(h, b->ran.create(hipEventDisableTiming));
    HIP_TRY(h, hipEventRecord(b->ran, h->stream));
    return flush_gather(h);      // with the next kernel queued, put the requested gather of the previous run on its stream
}

namespace {

// device_calls = false, or a runtime that answers "deinitialised": only the host structures go.  That is decided
// here, once; the members' destructors obey it (t_device_calls).
int destroy_batch(tp_batch_t b, bool device_calls) {
    tp_handle_t h = b->h;
    if (device_calls && runtime_gone(hipSetDevice(h->device))) device_calls = false;
    if (device_calls) {
        // A gather that was requested (tp_batch_gather_async) but not yet put on its stream is a collective the peer
        // ranks may already be waiting in: issue it before the buffers go away - dropping it would hang them.
        // (not at process exit: the peers may be gone, and a collective nobody answers would hang the exit)
        if (h->deferred == b && !g_exiting.load()) (void)flush_gather(h);
        (void)hipStreamSynchronize(h->stream);      // every launch of the batch went onto the kernel stream
        if (h->comm_stream) (void)hipStreamSynchronize(h->comm_stream);   // a gather may still read the results
        if (b->upload_done) (void)hipEventSynchronize(b->upload_done);    // copies may still write the inputs
    }
    if (h->deferred == b) h->deferred = nullptr;
    t_device_calls = device_calls;
    delete b;                                       // events and device memory go with their members
    t_device_calls = true;
    return TP_OK;
}

int destroy_handle(tp_handle_t h, bool device_calls) {
    if (device_calls && runtime_gone(hipSetDevice(h->device))) device_calls = false;
    // batches the caller left alive go first: they hold device memory, events and possibly a requested gather
    std::vector<tp_batch_t> left;
    left.swap(h->batches);
    for (tp_batch_t b : left) (void)destroy_batch(b, device_calls);
    if (device_calls) {
        if (h->comm_stream) (void)hipStreamSynchronize(h->comm_stream);
        if (h->stream) (void)hipStreamSynchronize(h->stream);
        if (h->comm) { (void)ncclCommDestroy(h->comm); h->comm = nullptr; }   // the communicator before its streams
    }
    t_device_calls = device_calls;
    delete h;                                       // streams and events, the kernel stream last (see tp_handle_s)
    t_device_calls = true;
    return TP_OK;
}

}  // namespace

extern "C" {

const char* tp_version(void) { return "tangency-posterior 0.6.0 (gfx950, fp64 MFMA: one wavefront per window k<=143, two or four per window k<=239, tiled pipeline k<=2047 with shared daily and intraday block Grams)"; }

int tp_max_assets(void) { return tp_tiled_max_assets(); }

int tp_sweep_max_assets(void) { return tp_sweep_max_k(); }

int tp_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

const char* tp_last_error(tp_handle_t h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int tp_create(int device_id, tp_handle_t* out) {
    if (!out) return fail(nullptr, TP_ERR_INVALID, "out is NULL");
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n < 1)
        return fail(nullptr, TP_ERR_NO_DEVICE, "no HIP device available (%s); there is no CPU fallback",
                    e == hipSuccess ? "device count 0" : hipGetErrorString(e));
    if (device_id < 0 || device_id >= n) return fail(nullptr, TP_ERR_INVALID, "device %d out of range (0..%d)", device_id, n - 1);
    std::unique_ptr<tp_handle_s> owner(new (std::nothrow) tp_handle_s());   // a failure half-way frees what was made
    tp_handle_t h = owner.get();
    if (!h) return fail(nullptr, TP_ERR_INVALID, "out of host memory");
    h->device = device_id;
    HIP_TRY(nullptr, hipSetDevice(device_id));
    HIP_TRY(nullptr, hipGetDeviceProperties(&h->prop, device_id));
    if (strncmp(h->prop.gcnArchName, "gfx950", 6) != 0)
        return fail(nullptr, TP_ERR_NO_DEVICE, "device %d is %s; libtangency is built for gfx950 only", device_id,
                    h->prop.gcnArchName);
    HIP_TRY(nullptr, h->stream.create());
    HIP_TRY(nullptr, h->kernel_span.create());
    HIP_TRY(nullptr, h->region_span.create());
    // the environment is read here and nowhere else (see tp_handle_s::opts)
    h->opts.wave_kernel = env_int("TP_WAVE_KERNEL", -1);
    h->opts.tiled_wave = env_int("TP_TILED_WAVE", -1);
    if (h->opts.tiled_wave < -1 || h->opts.tiled_wave > 1) h->opts.tiled_wave = -1;   // outside -1 / 0 / 1: automatic
    h->opts.tiled_fuse = env_int("TP_TILED_FUSE", -1);
    h->no_shared_gram = getenv("TP_NO_SHARED_GRAM") != nullptr ? 1 : 0;
    h->tiled_arena_gib = env_int("TP_TILED_ARENA_GIB", 0);
    h->tiled_arena_mib = env_int("TP_TILED_ARENA_MIB", 0);
    h->phase_limit = env_int("TP_PHASE_LIMIT", 0);
    {
        std::lock_guard<std::mutex> lk(g_registry_mutex);
        if (!g_atexit_registered) { atexit(shutdown_at_exit); g_atexit_registered = true; }
        g_live_handles.push_back(h);
    }
    *out = owner.release();
    return TP_OK;
}

int tp_set_option(tp_handle_t h, const char* name, int value) {
    if (!h || !name) return TP_ERR_INVALID;
    const std::string n(name);
    if (n == "wave_kernel") h->opts.wave_kernel = value;
    else if (n == "tiled_wave") {
        if (value < -1 || value > 1) return fail(h, TP_ERR_INVALID, "tp_set_option: tiled_wave=%d is not -1, 0 or 1", value);
        h->opts.tiled_wave = value;
    }
    else if (n == "tiled_fuse") h->opts.tiled_fuse = value;
    else if (n == "wave_preload") {
        if (value < -1 || value > 1) return fail(h, TP_ERR_INVALID, "tp_set_option: wave_preload=%d is not -1, 0 or 1", value);
        h->opts.wave_preload = value;
    }
    else if (n == "shared_tables") {
        if (value < -1 || value > 1) return fail(h, TP_ERR_INVALID, "tp_set_option: shared_tables=%d is not -1, 0 or 1", value);
        h->shared_tables = value;
    }
    else if (n == "no_shared_gram") h->no_shared_gram = value != 0;
    else if (n == "tiled_arena_gib") h->tiled_arena_gib = value;
    else if (n == "tiled_arena_mib") h->tiled_arena_mib = value;
    else if (n == "hf_share_min_blocks") h->hf_share_min_blocks = value;
    else if (n == "sweep_chunk_windows") {
        if (value < 0) return fail(h, TP_ERR_INVALID, "tp_set_option: sweep_chunk_windows=%d < 0", value);
        h->sweep_chunk_windows = value;
    }
    else return fail(h, TP_ERR_INVALID, "tp_set_option: unknown option '%s'", name);
    return TP_OK;
}

int tp_get_option(tp_handle_t h, const char* name, int* value) {
    if (!h || !name || !value) return TP_ERR_INVALID;
    const std::string n(name);
    if (n == "wave_kernel") *value = h->opts.wave_kernel;
    else if (n == "tiled_wave") *value = h->opts.tiled_wave;
    else if (n == "tiled_fuse") *value = h->opts.tiled_fuse;
    else if (n == "wave_preload") *value = h->opts.wave_preload;
    else if (n == "shared_tables") *value = h->shared_tables;
    else if (n == "last_shared_tables") *value = h->last_launch.shared_tables;   // read-only: what the last run did
    else if (n == "no_shared_gram") *value = h->no_shared_gram;
    else if (n == "tiled_arena_gib") *value = h->tiled_arena_gib;
    else if (n == "tiled_arena_mib") *value = h->tiled_arena_mib;
    else if (n == "hf_share_min_blocks") *value = h->hf_share_min_blocks;
    else if (n == "sweep_chunk_windows") *value = h->sweep_chunk_windows;
    else return fail(h, TP_ERR_INVALID, "tp_get_option: unknown option '%s'", name);
    return TP_OK;
}

int tp_destroy(tp_handle_t h) {
    if (!h) return TP_OK;
    if (g_shut_down.load()) return TP_OK;           // the exit handler already took every live handle down (h is gone)
    {
        std::lock_guard<std::mutex> lk(g_registry_mutex);
        auto it = std::find(g_live_handles.begin(), g_live_handles.end(), h);
        if (it == g_live_handles.end()) return TP_OK;   // not (or no longer) a live handle: never touch it
        g_live_handles.erase(it);
    }
    return destroy_handle(h, true);
}

int tp_device_info(tp_handle_t h, char* name, int name_len, int* compute_units, int* clock_mhz, int64_t* hbm_bytes) {
    if (!h) return TP_ERR_INVALID;
    if (name && name_len > 0) { snprintf(name, (size_t)name_len, "%s (%s)", h->prop.name[0] ? h->prop.name : "AMD Instinct MI355X", h->prop.gcnArchName); }
    if (compute_units) *compute_units = h->prop.multiProcessorCount;
    if (clock_mhz) *clock_mhz = h->prop.clockRate / 1000;
    if (hbm_bytes) *hbm_bytes = (int64_t)h->prop.totalGlobalMem;
    return TP_OK;
}

int tp_log_returns(tp_handle_t h, const double* prices, int64_t price_rows, int32_t ld, const int32_t* num,
                   const int32_t* den, int64_t n_out, double* out) {
    if (!h) return TP_ERR_INVALID;
    if (!prices || !out || price_rows < 1 || ld < 1) return fail(h, TP_ERR_INVALID, "tp_log_returns: prices / out missing");
    if (!num) return fail(h, TP_ERR_INVALID, "tp_log_returns: num missing");
    int rc = validate_pairs(h, "ret", num, den, n_out, price_rows);
    if (rc != TP_OK) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    DevBuf dp, dn, dd, dout;                             // of this call: freed on every return path
    rc = put(h, dp, prices, sizeof(double) * (size_t)price_rows * ld, "prices");
    if (rc == TP_OK) rc = put(h, dn, num, sizeof(int32_t) * (size_t)n_out, "numerator rows");
    if (rc == TP_OK) rc = put(h, dd, den, sizeof(int32_t) * (size_t)n_out, "denominator rows");
    if (rc == TP_OK) rc = ensure(h, dout, sizeof(double) * (size_t)n_out * ld, "log-returns");
    if (rc != TP_OK) return rc;
    HIP_TRY(h, h->kernel_span.begin(h->stream));         // tp_last_timing().kernel_ms = this kernel
    hipError_t e = tp_log_return_rows_launch((const double*)dp.p, ld, (const int*)dn.p, (const int*)dd.p,
                                             (long long)n_out, (double*)dout.p, h->stream);
    if (e != hipSuccess) return fail(h, TP_ERR_HIP, "log-return kernel launch failed: %s", hipGetErrorString(e));
    HIP_TRY(h, h->kernel_span.end(h->stream));
    return download(h, {{out, dout.p, sizeof(double) * (size_t)n_out * ld}});
}

int tp_batch_create(tp_handle_t h, const tp_params_t* p, int64_t W, tp_batch_t* out) {
    if (!h || !out) return TP_ERR_INVALID;
    *out = nullptr;
    int rc = check_params(h, p, W);
    if (rc != TP_OK) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    tp_batch_t b = new (std::nothrow) tp_batch_s();
    if (!b) return fail(h, TP_ERR_INVALID, "out of host memory");
    b->h = h; b->p = *p; b->W = W;
    rc = ensure(h, b->weights, sizeof(double) * (size_t)W * p->k, "weights");
    if (rc == TP_OK) rc = ensure(h, b->status, sizeof(int32_t) * (size_t)W, "statuses");
    if (rc == TP_OK) rc = ensure(h, b->aux, sizeof(double) * (size_t)W * TP_AUX_STRIDE, "aux");
    if (rc != TP_OK) { destroy_batch(b, true); return rc; }
    h->batches.push_back(b);
    *out = b;
    return TP_OK;
}

int tp_batch_destroy(tp_batch_t b) {
    if (!b) return TP_OK;
    if (g_shut_down.load()) return TP_OK;           // destroyed with its handle by the exit handler
    tp_handle_t h = b->h;
    auto it = std::find(h->batches.begin(), h->batches.end(), b);
    if (it != h->batches.end()) h->batches.erase(it);
    return destroy_batch(b, true);
}

// H2D of one batch on stream `st`.  wait = true: the synchronous form (tp_batch_upload) on the kernel stream;
// wait = false: copies are only queued (pinned host memory makes them truly asynchronous), upload_done marks their end.
static int upload_common(tp_batch_t b, const tp_inputs_t* in, hipStream_t st, bool wait) {
    tp_handle_t h = b->h;
    const tp_params_t& p = b->p;
    const int64_t W = b->W;
    int rc = validate_inputs(h, p, W, in);
    if (rc != TP_OK) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    const bool conj = p.strategy == TP_STRATEGY_CONJUGATE;
    // a launch of THIS batch that is still running reads the buffers about to be overwritten: the copy stream waits
    // for it (other batches' launches on the kernel stream are what the copies are meant to run under)
    if (!wait && b->ran) HIP_TRY(h, hipStreamWaitEvent(st, b->ran, 0));
    // a synchronous upload while an asynchronous one is still copying into the same buffers: let that one finish first
    if (wait && b->upload_pending && b->upload_done) HIP_TRY(h, hipEventSynchronize(b->upload_done));
    // the synchronous form borrows the kernel span (an unread kernel time is lost); the asynchronous one reads the
    // previous asynchronous upload's span before its events are reused
    Span& span = wait ? h->kernel_span : h->copy_span;
    if (!wait) HIP_TRY(h, span.read(h->h2d_ms));
    HIP_TRY(h, span.begin(st));
#define PUT(buf, ptr, bytes) do { rc = put(h, b->buf, (ptr), (bytes), #buf, st); if (rc != TP_OK) return rc; } while (0)
    // panels: log-returns as given, or formed on the device from prices (returns_frontend.hip)
    auto panel_in = [&](DevBuf& dst, PriceStaging& fe, const double* src, int64_t rows, int ld,
                        const int32_t* num, const int32_t* den, int64_t n_out) -> int {
        if (!num) return put(h, dst, src, sizeof(double) * (size_t)rows * ld, "return panel", st);
        int r = put(h, fe.prices, src, sizeof(double) * (size_t)rows * ld, "price panel", st);
        if (r == TP_OK) r = put(h, fe.num, num, sizeof(int32_t) * (size_t)n_out, "numerator rows", st);
        if (r == TP_OK) r = put(h, fe.den, den, sizeof(int32_t) * (size_t)n_out, "denominator rows", st);
        if (r == TP_OK) r = ensure(h, dst, sizeof(double) * (size_t)n_out * ld, "return panel");
        if (r != TP_OK) return r;
        hipError_t e = tp_log_return_rows_launch((const double*)fe.prices.p, ld, (const int*)fe.num.p, (const int*)fe.den.p,
                                                 (long long)n_out, (double*)dst.p, st);
        if (e != hipSuccess) return fail(h, TP_ERR_HIP, "log-return kernel launch failed: %s", hipGetErrorString(e));
        return TP_OK;
    };
    rc = panel_in(b->panel, b->fe, in->panel, in->panel_rows, in->panel_ld, in->ret_num,
                  in->ret_den, in->ret_rows);
    if (rc != TP_OK) return rc;
    PUT(start, in->start, sizeof(int64_t) * (size_t)W);
    PUT(row_idx, in->row_idx, sizeof(int32_t) * (size_t)W * p.n_r);
    PUT(n_rows, in->n_rows, sizeof(int32_t) * (size_t)W);
    PUT(col_idx, in->col_idx, sizeof(int32_t) * (size_t)W * p.k);
    PUT(rf_adj, in->rf_adj, sizeof(double) * (size_t)W * p.n_r);
    if (conj) {
        rc = panel_in(b->hf_panel, b->fe_hf, in->hf_panel, in->hf_rows, in->hf_ld,
                      in->hf_ret_num, in->hf_ret_den, in->hf_ret_rows);
        if (rc != TP_OK) return rc;
        PUT(hf_start, in->hf_start, sizeof(int64_t) * (size_t)W);
        PUT(hf_row_idx, in->hf_row_idx, sizeof(int32_t) * (size_t)W * p.m);
        PUT(hf_count, in->hf_count, sizeof(int32_t) * (size_t)W);
        PUT(w0, in->w0, sizeof(double) * (size_t)W * p.k);
        PUT(n0, in->n0, sizeof(double) * (size_t)W);
    }
#undef PUT
    b->panel_ld = in->panel_ld;
    b->hf_ld = conj ? in->hf_ld : 0;
    rc = plan_shared_gram(b, in, st);
    if (rc != TP_OK) return rc;
    plan_shared_hf(b, in);
    HIP_TRY(h, span.end(st));
    if (wait) {
        HIP_TRY(h, span.read(h->h2d_ms));
        b->fe = PriceStaging{};                        // needed only until the return panels exist
        b->fe_hf = PriceStaging{};
        b->upload_pending = false;
    } else {
        HIP_TRY(h, b->upload_done.create(hipEventDisableTiming));
        HIP_TRY(h, hipEventRecord(b->upload_done, st));
        b->upload_pending = true;
    }
    b->uploaded = true;
    return TP_OK;
}

int tp_batch_upload(tp_batch_t b, const tp_inputs_t* in) {
    if (!b) return TP_ERR_INVALID;
    return upload_common(b, in, b->h->stream, true);
}

int tp_batch_upload_async(tp_batch_t b, const tp_inputs_t* in) {
    if (!b) return TP_ERR_INVALID;
    tp_handle_t h = b->h;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, h->copy_stream.create());
    HIP_TRY(h, h->copy_span.create());
    return upload_common(b, in, h->copy_stream, false);
}

int tp_batch_upload_wait(tp_batch_t b) {
    if (!b) return TP_ERR_INVALID;
    tp_handle_t h = b->h;
    if (!b->upload_done) return TP_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipEventSynchronize(b->upload_done));
    if (!h->copy_span.busy()) HIP_TRY(h, h->copy_span.read(h->h2d_ms));
    return TP_OK;
}

// Page-locked host memory for panels and results: hipMemcpyAsync from / to it is a real DMA at PCIe rate and does
// not block the calling thread (pageable buffers are staged through the runtime's own bounce buffers at about half
// the rate).
int tp_host_alloc(void** out, int64_t bytes) {
    if (!out || bytes < 0) return TP_ERR_INVALID;
    *out = nullptr;
    if (hipHostMalloc(out, (size_t)(bytes > 0 ? bytes : 1), hipHostMallocDefault) != hipSuccess) { *out = nullptr; return TP_ERR_HIP; }
    return TP_OK;
}

int tp_host_free(void* p) {
    if (!p) return TP_OK;
    if (g_shut_down.load()) return TP_OK;           // after the exit handler: no call into a runtime that is shutting down
    return hipHostFree(p) == hipSuccess ? TP_OK : TP_ERR_HIP;
}

// 32-bit addressing of the staging loads: row x (8 ld) as a 24 x 24 bit product that fits 32 bits
int tp_addressing_flags(int64_t panel_bytes, int32_t ld, int32_t rows_per_window) {
    const size_t bytes = (size_t)panel_bytes;
    if (ld < 1 || (size_t)ld * 8 >= (1u << 24)) return 0;
    const size_t rows = bytes / ((size_t)ld * 8);
    int f = 0;
    if (bytes < (1ull << 32) && rows < (1u << 24)) f |= 1;
    // + 64: the lean loop advances its row offset one chunk past the window before it is clamped
    if (((size_t)rows_per_window + 64) * ld * 8 < (1ull << 32) && (size_t)rows_per_window < (1u << 24)) f |= 2;
    return f;
}

int tp_batch_addressing(tp_batch_t b, int* panel_flags, int* hf_flags) {
    if (!b) return TP_ERR_INVALID;
    if (panel_flags) *panel_flags = tp_addressing_flags((int64_t)b->panel.bytes, b->panel_ld, b->p.n_r);
    if (hf_flags) *hf_flags = b->hf_panel.p ? tp_addressing_flags((int64_t)b->hf_panel.bytes, b->hf_ld, b->p.m) : 0;
    return TP_OK;
}

int tp_batch_shared_gram_blocks(tp_batch_t b) { return b ? b->prefix_nblk : 0; }
int tp_batch_shared_intraday_blocks(tp_batch_t b) { return (b && b->hf_B > 0) ? b->hf_L : 0; }

// replace (src = NULL: drop) an optional per-window input; done when the call returns
static int replace_input(tp_batch_t b, DevBuf& buf, const void* src, size_t bytes, const char* what) {
    tp_handle_t h = b->h;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));       // a running launch may still read the old one
    int rc = put(h, buf, src, bytes, what);
    if (rc != TP_OK) return rc;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return TP_OK;
}

int tp_batch_set_rhs(tp_batch_t b, const double* rhs) {
    if (!b) return TP_ERR_INVALID;
    return replace_input(b, b->rhs, rhs, sizeof(double) * (size_t)b->W * b->p.k, "right-hand sides");
}

int tp_batch_set_shift(tp_batch_t b, const double* shift) {
    if (!b) return TP_ERR_INVALID;
    tp_handle_t h = b->h;
    if (shift && b->p.strategy != TP_STRATEGY_JEFFREYS)
        return fail(h, TP_ERR_INVALID, "tp_batch_set_shift applies to the Jeffreys strategy only");
    if (shift)
        for (int64_t i = 0; i < 2 * b->W; ++i)
            if (!(shift[i] >= 0.0) || !std::isfinite(shift[i]))
                return fail(h, TP_ERR_INVALID, "tp_batch_set_shift: shift[%lld] must be finite and >= 0", (long long)i);
    return replace_input(b, b->shift, shift, sizeof(double) * 2 * (size_t)b->W, "shifts");
}

int tp_batch_download_rhs(tp_batch_t b, double* rhs_out) {
    if (!b || !rhs_out) return TP_ERR_INVALID;
    tp_handle_t h = b->h;
    if (!b->uploaded) return fail(h, TP_ERR_INVALID, "tp_batch_download_rhs before tp_batch_upload");
    HIP_TRY(h, hipSetDevice(h->device));
    if (!b->out_rhs.p || !b->rhs_valid)
        return fail(h, TP_ERR_INVALID, "tp_batch_download_rhs: call tp_batch_keep_rhs before the tp_batch_run whose "
                                       "right-hand sides are wanted");
    return download(h, {{rhs_out, b->out_rhs.p, sizeof(double) * (size_t)b->W * b->p.k}});
}

int tp_batch_keep_rhs(tp_batch_t b, int on) {
    if (!b) return TP_ERR_INVALID;
    tp_handle_t h = b->h;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));       // a running launch may still write the old buffer
    b->rhs_valid = false;
    if (!on) { b->out_rhs.release(); return TP_OK; }
    return ensure(h, b->out_rhs, sizeof(double) * (size_t)b->W * b->p.k, "kept right-hand sides");
}

int tp_batch_keep_posterior(tp_batch_t b, int64_t w_begin, int64_t w_count) {
    if (!b) return TP_ERR_INVALID;
    tp_handle_t h = b->h;
    if (w_begin < 0 || w_count < 0 || w_begin > b->W || w_count > b->W - w_begin)
        return fail(h, TP_ERR_INVALID, "tp_batch_keep_posterior: windows [%lld, %lld + %lld) outside the batch's %lld",
                    (long long)w_begin, (long long)w_begin, (long long)w_count, (long long)b->W);
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));       // a running launch may still write the old buffer
    b->post_valid = false;
    b->post.release();                                 // first: the new buffer has exactly the size asked for
    b->post_w0 = 0;
    b->post_count = 0;
    if (w_count == 0) return TP_OK;
    int rc = ensure(h, b->post, sizeof(double) * (size_t)w_count * (size_t)b->p.k * (size_t)b->p.k, "tp_batch_keep_posterior: kept matrices");
    if (rc != TP_OK) return rc;
    b->post_w0 = w_begin;
    b->post_count = w_count;
    return TP_OK;
}

int tp_batch_download_posterior(tp_batch_t b, double* M) {
    if (!b) return TP_ERR_INVALID;
    tp_handle_t h = b->h;
    HIP_TRY(h, hipSetDevice(h->device));
    if (!b->post.p || !b->post_valid)
        return fail(h, TP_ERR_INVALID, "tp_batch_download_posterior: call tp_batch_keep_posterior before the tp_batch_run "
                                       "whose matrices are wanted");
    if (!M) return fail(h, TP_ERR_INVALID, "tp_batch_download_posterior: M is NULL");
    return download(h, {{M, b->post.p, sizeof(double) * (size_t)b->post_count * (size_t)b->p.k * (size_t)b->p.k}});
}

int tp_batch_run(tp_batch_t b) {
    if (!b) return TP_ERR_INVALID;
    tp_handle_t h = b->h;
    if (!b->uploaded) return fail(h, TP_ERR_INVALID, "tp_batch_run before tp_batch_upload");
    int rc = begin_launches(b);
    if (rc != TP_OK) return rc;
    if (b->out_rhs.p) b->rhs_valid = true;
    if (b->post.p) b->post_valid = true;
    if (b->pingpong) {
        b->parity ^= 1;
        if (b->gather_pending[b->parity]) {
            // The gather issued one run ago read this pair.  The HOST waits for it (the kernel of the previous run
            // is still executing, so the GPU does not idle): no stream of this library ever waits for another
            // stream's event on the device - such cross-queue waits cost ~0.1 ms per step (measured).
            HIP_TRY(h, hipEventSynchronize(b->gather_done[b->parity]));
            b->gather_pending[b->parity] = false;
        }
    }
    tp_kargs_t a = make_kargs(b);
    rc = launch(b, a, b->W, true);
    if (rc != TP_OK) return rc;
    b->has_run = true;
    return end_launches(b);
}

int tp_synchronize(tp_handle_t h) {
    if (!h) return TP_ERR_INVALID;
    HIP_TRY(h, hipSetDevice(h->device));
    int rcf = flush_gather(h);
    if (rcf != TP_OK) return rcf;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (h->comm_stream) {
        HIP_TRY(h, hipStreamSynchronize(h->comm_stream));
        HIP_TRY(h, h->gather_span.read(h->gather_ms));
    }
    return harvest_kernel_time(h);
}

int tp_batch_download(tp_batch_t b, double* weights, int32_t* status, double* aux) {
    if (!b) return TP_ERR_INVALID;
    tp_handle_t h = b->h;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    int rc = harvest_kernel_time(h);
    if (rc != TP_OK) return rc;
    HIP_TRY(h, h->kernel_span.begin(h->stream));       // (just read) around the copies, for d2h_ms
    if (weights) HIP_TRY(h, hipMemcpyAsync(weights, b->out_weights(), sizeof(double) * (size_t)b->W * b->p.k, hipMemcpyDeviceToHost, h->stream));
    if (status) HIP_TRY(h, hipMemcpyAsync(status, b->out_status(), sizeof(int32_t) * (size_t)b->W, hipMemcpyDeviceToHost, h->stream));
    if (aux) HIP_TRY(h, hipMemcpyAsync(aux, b->aux.p, sizeof(double) * (size_t)b->W * TP_AUX_STRIDE, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, h->kernel_span.end(h->stream));
    HIP_TRY(h, h->kernel_span.read(h->d2h_ms));
    return TP_OK;
}

int tp_batch_download_matrix(tp_batch_t b, int64_t w, int what, double* M, double* rhs) {
    if (!b || !M) return TP_ERR_INVALID;
    tp_handle_t h = b->h;
    if (!b->uploaded) return fail(h, TP_ERR_INVALID, "tp_batch_download_matrix before tp_batch_upload");
    if (w < 0 || w >= b->W) return fail(h, TP_ERR_INVALID, "window %lld out of range", (long long)w);
    if (what < TP_MATRIX_PRIOR || what > TP_MATRIX_POSTERIOR) return fail(h, TP_ERR_INVALID, "unknown matrix id %d", what);
    if (what == TP_MATRIX_PRIOR && b->p.strategy != TP_STRATEGY_CONJUGATE)
        return fail(h, TP_ERR_INVALID, "the prior scatter exists for the conjugate strategy only");
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t kk = (size_t)b->p.k * b->p.k;
    int rc = ensure(h, b->dbg, sizeof(double) * (kk + b->p.k), "matrix read-back");
    if (rc != TP_OK) return rc;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    rc = harvest_kernel_time(h);
    if (rc != TP_OK) return rc;
    HIP_TRY(h, hipMemsetAsync(b->dbg.p, 0, sizeof(double) * (kk + b->p.k), h->stream));
    tp_kargs_t a = make_kargs(b);
    a.dbg_S1 = (double*)b->dbg.p;
    a.out_post = nullptr;                              // the kept matrices are those of the last tp_batch_run
    a.post_count = 0;
    a.dbg_w = w;
    a.dbg_mode = what;
    a.w_first = w;
    a.w_count = 1;
    rc = launch(b, a, 1, false);
    if (rc != TP_OK) return rc;
    return download(h, {{M, b->dbg.p, sizeof(double) * kk}, {rhs, (double*)b->dbg.p + kk, sizeof(double) * b->p.k}});
}

int tp_batch_download_S1(tp_batch_t b, int64_t w, double* S1) {
    return tp_batch_download_matrix(b, w, TP_MATRIX_POSTERIOR, S1, nullptr);
}

int tp_batch_debug_stamps(tp_batch_t b, int64_t* stamps) {
    if (!b || !stamps) return TP_ERR_INVALID;
    tp_handle_t h = b->h;
#ifdef TP_STAMP
    HIP_TRY(h, hipSetDevice(h->device));
    int rc = ensure(h, b->stamps, sizeof(int64_t) * (size_t)b->W * 40, "phase stamps");
    if (rc != TP_OK) return rc;
    HIP_TRY(h, hipMemsetAsync(b->stamps.p, 0, sizeof(int64_t) * (size_t)b->W * 40, h->stream));
    rc = tp_batch_run(b);
    if (rc != TP_OK) return rc;
    return download(h, {{stamps, b->stamps.p, sizeof(int64_t) * (size_t)b->W * 40}});
#else
    return fail(h, TP_ERR_UNSUPPORTED, "libtangency was built without TP_STAMP (diagnostic phase stamps)");
#endif
}

int tp_posterior_batch(tp_handle_t h, const tp_params_t* p, int64_t W, const tp_inputs_t* in, double* weights,
                       int32_t* status, double* aux) {
    tp_batch_t b = nullptr;
    int rc = tp_batch_create(h, p, W, &b);
    if (rc != TP_OK) return rc;
    rc = tp_batch_upload(b, in);
    if (rc == TP_OK) rc = tp_batch_run(b);
    if (rc == TP_OK) rc = tp_batch_download(b, weights, status, aux);
    tp_batch_destroy(b);
    return rc;
}

int tp_last_timing(tp_handle_t h, double* kernel_ms, double* h2d_ms, double* d2h_ms, double* gather_ms) {
    if (!h) return TP_ERR_INVALID;
    if (kernel_ms) *kernel_ms = h->kernel_ms;
    if (h2d_ms) *h2d_ms = h->h2d_ms;
    if (d2h_ms) *d2h_ms = h->d2h_ms;
    if (gather_ms) *gather_ms = h->gather_ms;
    return TP_OK;
}

int tp_region_begin(tp_handle_t h) {
    if (!h) return TP_ERR_INVALID;
    HIP_TRY(h, hipSetDevice(h->device));
    if (h->ring.empty()) {
        std::vector<Span> ring(TP_REGION_MAX_STEPS);   // kept only when every span exists
        for (Span& s : ring) HIP_TRY(h, s.create());
        h->ring.swap(ring);
    }
    h->ring_used = 0;
    h->step_ms.clear();
    h->in_region = true;
    HIP_TRY(h, h->region_span.begin(h->stream));
    return TP_OK;
}

int tp_region_end(tp_handle_t h, double* ms) {
    if (!h) return TP_ERR_INVALID;
    HIP_TRY(h, hipSetDevice(h->device));
    h->in_region = false;
    HIP_TRY(h, h->region_span.end(h->stream));
    double whole = 0;
    HIP_TRY(h, h->region_span.read(whole));
    if (ms) *ms = whole;
    for (int i = 0; i < h->ring_used; ++i) {
        double step = 0;
        HIP_TRY(h, h->ring[(size_t)i].read(step));
        h->step_ms.push_back(step);
    }
    if (!h->step_ms.empty()) h->kernel_ms = h->step_ms.back();
    return harvest_kernel_time(h);
}

int tp_region_steps(tp_handle_t h, double* step_ms, int capacity, int* n_steps) {
    if (!h || !n_steps || capacity < 0) return TP_ERR_INVALID;
    const int n = (int)h->step_ms.size();
    *n_steps = n;
    if (step_ms)
        for (int i = 0; i < n && i < capacity; ++i) step_ms[i] = h->step_ms[(size_t)i];
    return TP_OK;
}

int tp_last_launch(tp_handle_t h, int* grid, int* block, int* lds_bytes, int* ntile) {
    if (!h) return TP_ERR_INVALID;
    if (grid) *grid = h->last_launch.grid;
    if (block) *block = h->last_launch.block;
    if (lds_bytes) *lds_bytes = h->last_launch.lds_bytes;
    if (ntile) *ntile = h->last_launch.ntile;
    return TP_OK;
}

}  // extern "C"
