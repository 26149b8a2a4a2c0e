// tangency_replay.cpp - the backtest replay of the C-ABI of libtangency.so (include/tangency_posterior.h):
// tp_replay_merge_maps (host only), tp_replay_run, tp_replay_run_batch, tp_replay_download, and the summary of a run's returns
// over a grid of trading costs, tp_replay_summary / tp_replay_download_summary (replay_summary.hip).  A run is: checks of every offset,
// stride and index on the host, the merge maps of every distinct universe table, the uploads, then one launch per
// slots-per-lane class of the portfolios inside one timed span (backtest_replay.hip).  The buffers live on the handle (ReplayWs,
// tangency_host.h).  tp_replay_run_batch is the same run with the weights left where a batch's run or sweep wrote them.
#include <cmath>
#include <cstring>
#include <algorithm>
#include <map>
#include <tuple>
#include <vector>

#include "tangency_host.h"

using namespace tp_host;

static_assert(TP_REPLAY_SUM_CHECK == TP_REPLAY_KSTATUS_SUM_CHECK, "replay status codes out of sync");
static_assert(TP_REPLAY_BAD_WEIGHTS == TP_REPLAY_KSTATUS_BAD_WEIGHTS, "replay status codes out of sync");
static_assert(TP_SUMMARY_STATS == TP_SUMMARY_NSTATS, "summary record sizes out of sync");
static_assert(TP_SUMMARY_NO_REPLAY == TP_SUMMARY_KSTATUS_NO_REPLAY && TP_SUMMARY_NONFINITE == TP_SUMMARY_KSTATUS_NONFINITE,
              "summary status codes out of sync");

namespace {

// rows [0, R) of `k` elements at `off + j * stride` inside a buffer of `len` elements, without overflow
bool rows_fit(int64_t off, int64_t stride, int64_t R, int64_t k, int64_t len) {
    if (off < 0 || stride < 0 || k > len || off > len - k) return false;
    return R <= 1 || stride <= (len - k - off) / (R - 1);
}

// the maps of ONE universe table; `pos` is a scratch table of K entries, all -1 on entry and on return
int merge_maps(tp_handle_t h, const int32_t* cols, int64_t R, int32_t k, int64_t stride, int32_t K, int32_t* prev_slot,
               int32_t* next_slot, std::vector<int32_t>& pos) {
    int rc = TP_OK;
    for (int64_t j = 0; j < R && rc == TP_OK; ++j) {
        const int32_t* cur = cols + j * stride;
        for (int32_t i = 0; i < k; ++i)
            if (cur[i] < 0 || cur[i] >= K)
                return fail(h, TP_ERR_INVALID, "tp_replay: column index %d at rebalancing date %lld, slot %d is outside [0, %d)",
                            cur[i], (long long)j, i, K);
        // the slots of date j, looked up by the rows before and after it
        int32_t filled = 0;
        for (; filled < k; ++filled) {
            if (pos[(size_t)cur[filled]] != -1) {
                rc = fail(h, TP_ERR_INVALID, "tp_replay: ticker %d is held twice at rebalancing date %lld", cur[filled], (long long)j);
                break;
            }
            pos[(size_t)cur[filled]] = filled;
        }
        if (rc == TP_OK) {
            if (j > 0) {
                const int32_t* before = cols + (j - 1) * stride;
                for (int32_t i = 0; i < k; ++i) next_slot[(j - 1) * k + i] = pos[(size_t)before[i]];
            }
            if (j + 1 < R) {
                const int32_t* after = cols + (j + 1) * stride;
                for (int32_t i = 0; i < k; ++i) {
                    const int32_t c = after[i];
                    prev_slot[(j + 1) * k + i] = (c >= 0 && c < K) ? pos[(size_t)c] : -1;   // (row j+1 is checked in its own turn)
                }
            }
        }
        for (int32_t i = 0; i < filled; ++i) pos[(size_t)cur[i]] = -1;
    }
    if (rc != TP_OK) return rc;
    for (int32_t i = 0; i < k; ++i) { prev_slot[i] = -1; next_slot[(R - 1) * k + i] = -1; }
    return TP_OK;
}

int check_maps_args(tp_handle_t h, const int32_t* cols, int64_t R, int32_t k, int64_t stride, int32_t K) {
    if (!cols) return fail(h, TP_ERR_INVALID, "tp_replay: cols is NULL");
    if (R < 1) return fail(h, TP_ERR_INVALID, "tp_replay: R=%lld < 1", (long long)R);
    if (k < 1) return fail(h, TP_ERR_INVALID, "tp_replay: k=%d < 1", k);
    if (K < 1) return fail(h, TP_ERR_INVALID, "tp_replay: K=%d < 1", K);
    if (stride < 0) return fail(h, TP_ERR_INVALID, "tp_replay: stride=%lld < 0", (long long)stride);
    if (R > INT64_MAX / 8 / k) return fail(h, TP_ERR_INVALID, "tp_replay: R x k overflows");
    return TP_OK;
}

int upload(tp_handle_t h, DevBuf& b, const void* src, size_t bytes, const char* what) {
    const int rc = ensure(h, b, bytes, what);
    if (rc != TP_OK) return rc;
    if (bytes) HIP_TRY(h, hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, h->stream));
    return TP_OK;
}

// What tp_replay_run_batch adds to a run: the source's results on the device and their counts, the scales, the status
// offsets and the patches (host arrays).
struct Feed {
    const double* src_weights;
    const int32_t* src_status;
    int64_t status_len;
    const double* w_scale;
    const int64_t* s_off;
    const int64_t* s_stride;
    int64_t n_patch;
    const int64_t* patch_port;
    const int32_t* patch_date;
    const double* patch_weights;
    int32_t patch_ld;
};

// tp_replay_run (`feed` == NULL: `weights` is the caller's host array) and tp_replay_run_batch (`weights` is not read: the
// kernel takes feed->src_weights, of weights_len elements) on the handle `h`; `name` is the entry point, for the messages
int run_replay(tp_handle_t h, const char* name, int64_t D, int32_t ld, const double* S, const double* rf_daily, int64_t R,
               const int32_t* reb_day, int32_t K, int64_t P, const int32_t* k, const double* scaling, const double* cost,
               const int64_t* w_off, const int64_t* w_stride, const int64_t* u_off, const int64_t* u_stride,
               const double* weights, int64_t weights_len, const int32_t* cols, const double* caps, int64_t universe_len,
               const Feed* feed) {
    ReplayWs& ws = h->replay;
    // ---- checks: nothing below them reads outside a caller's array, on the host or on the device
    if (D < 1 || D > 0x7fffffffLL) return fail(h, TP_ERR_INVALID, "%s: D=%lld outside [1, 2^31)", name, (long long)D);
    if (R < 1 || R > D) return fail(h, TP_ERR_INVALID, "%s: R=%lld outside [1, D=%lld]", name, (long long)R, (long long)D);
    if (P < 0 || P > 0x7fffffffLL) return fail(h, TP_ERR_INVALID, "%s: P=%lld outside [0, 2^31)", name, (long long)P);
    if (ld < 1 || K < 1 || K > ld) return fail(h, TP_ERR_INVALID, "%s: ld=%d, K=%d: 1 <= K <= ld expected", name, ld, K);
    if (weights_len < 0 || universe_len < 0) return fail(h, TP_ERR_INVALID, "%s: a negative buffer length", name);
    if (!S || !rf_daily || !reb_day) return fail(h, TP_ERR_INVALID, "%s: S, rf_daily or reb_day is NULL", name);
    if (P > 0 && (!k || !scaling || !cost || !w_off || !w_stride || !u_off || !u_stride || (!feed && !weights) || !cols || !caps))
        return fail(h, TP_ERR_INVALID, "%s: a per-portfolio array or a flat buffer is NULL", name);
    if (feed && P > 0 && (!feed->s_off || !feed->s_stride)) return fail(h, TP_ERR_INVALID, "%s: s_off or s_stride is NULL", name);
    if (reb_day[0] != 0) return fail(h, TP_ERR_INVALID, "%s: reb_day[0]=%d, the first trading day rebalances", name, reb_day[0]);
    for (int64_t j = 1; j < R; ++j)
        if (reb_day[j] <= reb_day[j - 1] || reb_day[j] >= D)
            return fail(h, TP_ERR_INVALID, "%s: reb_day[%lld]=%d is not strictly increasing below D=%lld", name, (long long)j,
                        reb_day[j], (long long)D);
    for (int64_t p = 0; p < P; ++p) {
        if (k[p] < 1) return fail(h, TP_ERR_INVALID, "%s: k[%lld]=%d < 1", name, (long long)p, k[p]);
        if (k[p] > tp_max_assets())
            return fail(h, TP_ERR_UNSUPPORTED, "%s: k[%lld]=%d exceeds the largest supported universe %d", name, (long long)p,
                        k[p], tp_max_assets());
        if (!rows_fit(w_off[p], w_stride[p], R, k[p], weights_len))
            return fail(h, TP_ERR_INVALID, "%s: portfolio %lld: w_off=%lld, w_stride=%lld run past the %lld weights",
                        name, (long long)p, (long long)w_off[p], (long long)w_stride[p], (long long)weights_len);
        if (feed && !rows_fit(feed->s_off[p], feed->s_stride[p], R, 1, feed->status_len))
            return fail(h, TP_ERR_INVALID, "%s: portfolio %lld: s_off=%lld, s_stride=%lld run past the %lld statuses",
                        name, (long long)p, (long long)feed->s_off[p], (long long)feed->s_stride[p], (long long)feed->status_len);
        if (!rows_fit(u_off[p], u_stride[p], R, k[p], universe_len))
            return fail(h, TP_ERR_INVALID, "%s: portfolio %lld: u_off=%lld, u_stride=%lld run past the %lld universe entries",
                        name, (long long)p, (long long)u_off[p], (long long)u_stride[p], (long long)universe_len);
    }
    // the patches: sorted by (portfolio, date), so every portfolio's are one range [first[p], first[p + 1])
    std::vector<int32_t> patch_first;
    if (feed) {
        const int64_t n = feed->n_patch;
        if (n < 0 || n > 0x7fffffffLL) return fail(h, TP_ERR_INVALID, "%s: n_patch=%lld outside [0, 2^31)", name, (long long)n);
        if (n > 0 && (!feed->patch_port || !feed->patch_date || !feed->patch_weights))
            return fail(h, TP_ERR_INVALID, "%s: patch_port, patch_date or patch_weights is NULL", name);
        patch_first.assign((size_t)P + 1, 0);
        for (int64_t q = 0; q < n; ++q) {
            const int64_t pp = feed->patch_port[q];
            const int32_t pj = feed->patch_date[q];
            if (pp < 0 || pp >= P) return fail(h, TP_ERR_INVALID, "%s: patch_port[%lld]=%lld outside [0, P=%lld)", name, (long long)q, (long long)pp, (long long)P);
            if (pj < 0 || pj >= R) return fail(h, TP_ERR_INVALID, "%s: patch_date[%lld]=%d outside [0, R=%lld)", name, (long long)q, pj, (long long)R);
            if (q > 0 && (pp < feed->patch_port[q - 1] || (pp == feed->patch_port[q - 1] && pj <= feed->patch_date[q - 1])))
                return fail(h, TP_ERR_INVALID, "%s: patch %lld (portfolio %lld, date %d) is not after patch %lld: sorted by (portfolio, date), "
                            "strictly increasing, expected", name, (long long)q, (long long)pp, pj, (long long)(q - 1));
            if (feed->patch_ld < k[pp])
                return fail(h, TP_ERR_INVALID, "%s: patch_ld=%d is smaller than k[%lld]=%d of a patched portfolio", name, feed->patch_ld, (long long)pp, k[pp]);
            ++patch_first[(size_t)pp + 1];
        }
        for (int64_t p = 0; p < P; ++p) patch_first[(size_t)p + 1] += patch_first[(size_t)p];
    }
    // ---- merge maps, once per distinct universe table (they validate the column indices), and the portfolios by class
    std::map<std::tuple<int64_t, int64_t, int32_t>, int64_t> tables;
    std::vector<int32_t> prev, next, pos((size_t)K, -1);
    std::vector<tp_replay_port_t> port((size_t)P);
    for (int64_t p = 0; p < P; ++p) {
        const auto key = std::make_tuple(u_off[p], u_stride[p], k[p]);
        auto it = tables.find(key);
        if (it == tables.end()) {
            int rc = check_maps_args(h, cols, R, k[p], u_stride[p], K);
            if (rc != TP_OK) return rc;
            const size_t at = prev.size(), n = (size_t)R * (size_t)k[p];
            prev.resize(at + n);
            next.resize(at + n);
            rc = merge_maps(h, cols + u_off[p], R, k[p], u_stride[p], K, prev.data() + at, next.data() + at, pos);
            if (rc != TP_OK) return rc;
            it = tables.emplace(key, (int64_t)at).first;
        }
        tp_replay_port_t& pt = port[(size_t)p];
        pt = tp_replay_port_t{w_off[p], w_stride[p], u_off[p], u_stride[p], it->second, scaling[p], cost[p], k[p], 0, 0, 0, 1.0, 0, 0};
        if (feed) {
            pt.s_off = feed->s_off[p]; pt.s_stride = feed->s_stride[p];
            pt.w_scale = feed->w_scale ? feed->w_scale[p] : 1.0;
            pt.patch_first = patch_first[(size_t)p]; pt.patch_end = patch_first[(size_t)p + 1];
        }
    }
    std::vector<int32_t> order((size_t)P);
    for (int64_t p = 0; p < P; ++p) order[(size_t)p] = (int32_t)p;
    std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) {
        return tp_replay_slots_per_lane(k[x]) < tp_replay_slots_per_lane(k[y]);
    });
    // ---- device: drain what was queued (the buffers may be in use, the span unread; a batch's sweep ends here), upload, launch
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    int rc = harvest_kernel_time(h);
    if (rc != TP_OK) return rc;
    ws.ran = false;
    ws.summarised = false;                                // (a summary belongs to the run it read)
    struct Up { DevBuf* b; const void* src; size_t bytes; const char* what; };
    const size_t flat = P > 0 ? 1 : 0;                    // (no portfolio: the flat buffers may be absent)
    const size_t n_patch = feed ? (size_t)feed->n_patch : 0;
    const Up ups[] = {
        {&ws.S, S, (size_t)D * (size_t)ld * sizeof(double), "replay returns"},
        {&ws.rf, rf_daily, (size_t)D * sizeof(double), "replay risk-free rates"},
        {&ws.reb, reb_day, (size_t)R * sizeof(int32_t), "replay rebalancing days"},
        {&ws.weights, weights, (feed ? 0 : flat) * (size_t)weights_len * sizeof(double), "replay weights"},
        {&ws.cols, cols, flat * (size_t)universe_len * sizeof(int32_t), "replay universes"},
        {&ws.caps, caps, flat * (size_t)universe_len * sizeof(double), "replay market caps"},
        {&ws.prev, prev.data(), prev.size() * sizeof(int32_t), "replay merge maps"},
        {&ws.next, next.data(), next.size() * sizeof(int32_t), "replay merge maps"},
        {&ws.port, port.data(), port.size() * sizeof(tp_replay_port_t), "replay portfolios"},
        {&ws.order, order.data(), order.size() * sizeof(int32_t), "replay launch order"},
        {&ws.patch_date, feed ? feed->patch_date : nullptr, n_patch * sizeof(int32_t), "replay patch dates"},
        {&ws.patch_rows, feed ? feed->patch_weights : nullptr, n_patch * (size_t)(feed ? feed->patch_ld : 0) * sizeof(double),
         "replay patch rows"},
    };
    for (const Up& u : ups)
        if ((rc = upload(h, *u.b, u.src, u.bytes, u.what)) != TP_OK) return rc;
    if ((rc = ensure(h, ws.ret, (size_t)P * (size_t)D * sizeof(double), "replay returns out")) != TP_OK) return rc;
    if ((rc = ensure(h, ws.turnover, (size_t)P * (size_t)R * sizeof(double), "replay turnover")) != TP_OK) return rc;
    if ((rc = ensure(h, ws.metrics, (size_t)P * (size_t)R * TP_REPLAY_METRICS * sizeof(double), "replay metrics")) != TP_OK) return rc;
    if ((rc = ensure(h, ws.status, (size_t)P * sizeof(int32_t), "replay status")) != TP_OK) return rc;
    if ((rc = ensure(h, ws.bad_day, (size_t)P * sizeof(int32_t), "replay days")) != TP_OK) return rc;
    HIP_TRY(h, hipStreamSynchronize(h->stream));          // the host arrays (the caller's and the ones above) are free again

    tp_replay_args_t a;
    memset(&a, 0, sizeof a);
    a.S = (const double*)ws.S.p; a.rf = (const double*)ws.rf.p; a.reb_day = (const int*)ws.reb.p;
    a.port = (const tp_replay_port_t*)ws.port.p; a.order = (const int*)ws.order.p;
    a.weights = (const double*)ws.weights.p; a.cols = (const int*)ws.cols.p; a.caps = (const double*)ws.caps.p;
    a.prev_slot = (const int*)ws.prev.p; a.next_slot = (const int*)ws.next.p;
    a.ret = (double*)ws.ret.p; a.turnover = (double*)ws.turnover.p; a.metrics = (double*)ws.metrics.p;
    a.status = (int*)ws.status.p; a.bad_day = (int*)ws.bad_day.p;
    a.D = (int)D; a.R = (int)R; a.ld = ld;
    if (feed) {                                           // (P > 0 passed the checks: the source has entries, its buffers exist)
        a.weights = feed->src_weights; a.src_status = (const int*)feed->src_status;
        a.patch_date = (const int*)ws.patch_date.p; a.patch_rows = (const double*)ws.patch_rows.p; a.patch_ld = feed->patch_ld;
    }
    const tp_launch_info_t keep_launch = h->last_launch;  // tp_last_launch keeps describing tp_batch_run
    Span& span = timed_span(h);
    HIP_TRY(h, span.begin(h->stream));
    for (int64_t first = 0; first < P;) {
        const int spl = tp_replay_slots_per_lane(k[order[(size_t)first]]);
        int64_t end = first;
        while (end < P && tp_replay_slots_per_lane(k[order[(size_t)end]]) == spl) ++end;
        a.first = (int)first; a.count = (int)(end - first);
        const hipError_t e = tp_replay_launch(a, spl, h->stream);
        if (e != hipSuccess) return fail(h, TP_ERR_HIP, "replay kernel launch failed: %s", hipGetErrorString(e));
        first = end;
    }
    h->last_launch = keep_launch;
    rc = timed_done(h, span);
    if (rc != TP_OK) return rc;
    ws.P = P; ws.D = D; ws.R = R;
    ws.h_reb.assign(reb_day, reb_day + R);
    ws.ran = true;
    return TP_OK;
}

}  // namespace

extern "C" {

int tp_replay_merge_maps(const int32_t* cols, int64_t R, int32_t k, int64_t stride, int32_t K, int32_t* prev_slot,
                         int32_t* next_slot) {
    int rc = check_maps_args(nullptr, cols, R, k, stride, K);
    if (rc != TP_OK) return rc;
    if (!prev_slot || !next_slot) return fail(nullptr, TP_ERR_INVALID, "tp_replay_merge_maps: prev_slot / next_slot is NULL");
    std::vector<int32_t> pos((size_t)K, -1);
    return merge_maps(nullptr, cols, R, k, stride, K, prev_slot, next_slot, pos);
}

int tp_replay_run(tp_handle_t h, int64_t D, int32_t ld, const double* S, const double* rf_daily, int64_t R,
                  const int32_t* reb_day, int32_t K, int64_t P, const int32_t* k, const double* scaling, const double* cost,
                  const int64_t* w_off, const int64_t* w_stride, const int64_t* u_off, const int64_t* u_stride,
                  const double* weights, int64_t weights_len, const int32_t* cols, const double* caps, int64_t universe_len) {
    if (!h) return TP_ERR_INVALID;
    return run_replay(h, "tp_replay_run", D, ld, S, rf_daily, R, reb_day, K, P, k, scaling, cost, w_off, w_stride, u_off, u_stride,
                      weights, weights_len, cols, caps, universe_len, nullptr);
}

int tp_replay_run_batch(tp_batch_t b, int source, int64_t D, int32_t ld, const double* S, const double* rf_daily, int64_t R,
                        const int32_t* reb_day, int32_t K, int64_t P, const int32_t* k, const double* scaling, const double* cost,
                        const double* w_scale, const int64_t* w_off, const int64_t* w_stride, const int64_t* s_off,
                        const int64_t* s_stride, const int64_t* u_off, const int64_t* u_stride, const int32_t* cols,
                        const double* caps, int64_t universe_len, int64_t n_patch, const int64_t* patch_port,
                        const int32_t* patch_date, const double* patch_weights, int32_t patch_ld) {
    if (!b) return TP_ERR_INVALID;
    tp_handle_t h = b->h;
    const char* name = "tp_replay_run_batch";
    // the source: where the batch's last call of that kind wrote, and how many entries (weight rows, statuses) it wrote
    Feed feed{nullptr, nullptr, 0, w_scale, s_off, s_stride, n_patch, patch_port, patch_date, patch_weights, patch_ld};
    int64_t per_window = 0;
    const char* producer = "";
    switch (source) {
        case TP_REPLAY_SRC_RUN:
            per_window = b->has_run ? 1 : 0; producer = "tp_batch_run";
            feed.src_weights = b->out_weights(); feed.src_status = b->out_status();
            break;
        case TP_REPLAY_SRC_PRIOR_SWEEP:
            per_window = b->ps.P < 1 ? 0 : (int64_t)b->ps.P * b->ps.S; producer = "tp_batch_prior_sweep";
            feed.src_weights = (const double*)b->ps.weights.p; feed.src_status = (const int32_t*)b->ps.status.p;
            break;
        case TP_REPLAY_SRC_SIZE_SWEEP:
            per_window = b->zs.P < 1 || b->zs.S < 1 ? 0 : (int64_t)b->zs.P * b->zs.S; producer = "tp_batch_size_sweep";
            feed.src_weights = (const double*)b->zs.weights.p; feed.src_status = (const int32_t*)b->zs.status.p;
            break;
        case TP_REPLAY_SRC_WINDOW_SWEEP:
            per_window = b->wn.P < 1 || b->wn.L < 1 ? 0 : (int64_t)b->wn.P * b->wn.L; producer = "tp_batch_window_sweep";
            feed.src_weights = (const double*)b->wn.weights.p; feed.src_status = (const int32_t*)b->wn.status.p;
            break;
        case TP_REPLAY_SRC_GRID_SWEEP:
            per_window = b->gr.P < 1 || b->gr.L < 1 || b->gr.S < 1 ? 0 : (int64_t)b->gr.P * b->gr.L * b->gr.S;
            producer = "tp_batch_grid_sweep";
            feed.src_weights = (const double*)b->gr.weights.p; feed.src_status = (const int32_t*)b->gr.status.p;
            break;
        case TP_REPLAY_SRC_SWEEP_FINISH:
            if (b->sw.finish_stale)
                return fail(h, TP_ERR_INVALID, "%s: a solve sweep after the last tp_batch_sweep_finish replaced the solutions it read "
                            "(source %d)", name, source);
            per_window = b->sw.finished ? 1 : 0; producer = "tp_batch_sweep_finish";
            feed.src_weights = (const double*)b->sw.fin_weights.p; feed.src_status = (const int32_t*)b->sw.fin_status.p;
            break;
        case TP_REPLAY_SRC_SPECTRAL:
            per_window = b->sp.S < 1 ? 0 : 1; producer = "tp_batch_spectral_greyserman";
            feed.src_weights = (const double*)b->sp.weights.p; feed.src_status = (const int32_t*)b->sp.status.p;
            break;
        default:
            return fail(h, TP_ERR_INVALID, "%s: unknown source %d", name, source);
    }
    if (per_window < 1) return fail(h, TP_ERR_INVALID, "%s: the batch has no results of source %d (no %s before it)", name, source, producer);
    feed.status_len = b->W * per_window;                  // (what the source's download copies: W x ... entries, k weights each)
    return run_replay(h, name, D, ld, S, rf_daily, R, reb_day, K, P, k, scaling, cost, w_off, w_stride, u_off, u_stride, nullptr,
                      feed.status_len * b->p.k, cols, caps, universe_len, &feed);
}

int tp_replay_download(tp_handle_t h, double* returns, double* turnover, double* metrics, int32_t* status, int32_t* bad_day) {
    if (!h) return TP_ERR_INVALID;
    const ReplayWs& ws = h->replay;
    if (!ws.ran) return fail(h, TP_ERR_INVALID, "tp_replay_download without a tp_replay_run or tp_replay_run_batch before it");
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t P = (size_t)ws.P, D = (size_t)ws.D, R = (size_t)ws.R;
    return download(h, {{returns, ws.ret.p, P * D * sizeof(double)},
                        {turnover, ws.turnover.p, P * R * sizeof(double)},
                        {metrics, ws.metrics.p, P * R * TP_REPLAY_METRICS * sizeof(double)},
                        {status, ws.status.p, P * sizeof(int32_t)},
                        {bad_day, ws.bad_day.p, P * sizeof(int32_t)}});
}

int tp_replay_summary(tp_handle_t h, int32_t C, const double* cost_bp, const double* rf_excess) {
    if (!h) return TP_ERR_INVALID;
    ReplayWs& ws = h->replay;
    // ---- checks, all before the drain: a refused call leaves the last replay's and the last summary's results in place
    if (!ws.ran) return fail(h, TP_ERR_INVALID, "tp_replay_summary without a tp_replay_run or tp_replay_run_batch before it");
    if (C < 1 || C > TP_SUMMARY_MAX_COSTS)
        return fail(h, TP_ERR_INVALID, "tp_replay_summary: C=%d outside [1, %d]", C, TP_SUMMARY_MAX_COSTS);
    if (!cost_bp || !rf_excess) return fail(h, TP_ERR_INVALID, "tp_replay_summary: cost_bp or rf_excess is NULL");
    for (int32_t c = 0; c < C; ++c)
        if (!std::isfinite(cost_bp[c])) return fail(h, TP_ERR_INVALID, "tp_replay_summary: cost_bp[%d] is not finite", c);
    if (ws.D < 2) return fail(h, TP_ERR_INVALID, "tp_replay_summary: D=%lld: a replay of at least two trading days (one return) is expected", (long long)ws.D);
    const size_t P = (size_t)ws.P, D = (size_t)ws.D, R = (size_t)ws.R;
    // the rebalancing date of every trading day (date 0, on day 0, charges nothing: ref:1212 needs a portfolio before it)
    std::vector<int32_t> day_date(D, -1);
    for (size_t j = 1; j < R; ++j) day_date[(size_t)ws.h_reb[j]] = (int32_t)j;
    // ---- device: drain (the replay ends here; its span is read), upload, one launch that is not awaited
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    int rc = harvest_kernel_time(h);
    if (rc != TP_OK) return rc;
    ws.summarised = false;
    if ((rc = upload(h, ws.sum_cost, cost_bp, (size_t)C * sizeof(double), "summary costs")) != TP_OK) return rc;
    if ((rc = upload(h, ws.sum_rf, rf_excess, D * sizeof(double), "summary excess risk-free rates")) != TP_OK) return rc;
    if ((rc = upload(h, ws.sum_day, day_date.data(), D * sizeof(int32_t), "summary days")) != TP_OK) return rc;
    if ((rc = ensure(h, ws.sum_stats, P * (size_t)C * TP_SUMMARY_STATS * sizeof(double), "summary records")) != TP_OK) return rc;
    if ((rc = ensure(h, ws.sum_status, P * (size_t)C * sizeof(int32_t), "summary statuses")) != TP_OK) return rc;
    HIP_TRY(h, hipStreamSynchronize(h->stream));          // the host arrays are free again
    tp_summary_args_t a;
    memset(&a, 0, sizeof a);
    a.ret = (const double*)ws.ret.p; a.turnover = (const double*)ws.turnover.p; a.rstatus = (const int*)ws.status.p;
    a.reb_day = (const int*)ws.reb.p; a.day_date = (const int*)ws.sum_day.p;
    a.cost_bp = (const double*)ws.sum_cost.p; a.rf_excess = (const double*)ws.sum_rf.p;
    a.stats = (double*)ws.sum_stats.p; a.status = (int*)ws.sum_status.p;
    a.P = (int)ws.P; a.D = (int)ws.D; a.R = (int)ws.R; a.C = C;
    const tp_launch_info_t keep_launch = h->last_launch;  // tp_last_launch keeps describing tp_batch_run
    Span& span = timed_span(h);
    HIP_TRY(h, span.begin(h->stream));
    const hipError_t e = tp_summary_launch(a, h->stream);
    if (e != hipSuccess) return fail(h, TP_ERR_HIP, "replay summary kernel launch failed: %s", hipGetErrorString(e));
    h->last_launch = keep_launch;
    rc = timed_done(h, span);
    if (rc != TP_OK) return rc;
    ws.C = C;
    ws.summarised = true;
    return TP_OK;
}

int tp_replay_download_summary(tp_handle_t h, double* stats, int32_t* status) {
    if (!h) return TP_ERR_INVALID;
    const ReplayWs& ws = h->replay;
    if (!ws.ran || !ws.summarised)
        return fail(h, TP_ERR_INVALID, "tp_replay_download_summary without a tp_replay_summary of the last replay before it");
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t n = (size_t)ws.P * (size_t)ws.C;
    return download(h, {{stats, ws.sum_stats.p, n * TP_SUMMARY_STATS * sizeof(double)},
                        {status, ws.sum_status.p, n * sizeof(int32_t)}});
}

}  // extern "C"
