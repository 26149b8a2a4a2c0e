// tangency_replay.cpp - the backtest replay of the C-ABI of libtangency.so (include/tangency_posterior.h):
// tp_replay_merge_maps (host only), tp_replay_run, tp_replay_download.  A run is: checks of every offset, stride and index
// on the host, the merge maps of every distinct universe table, the uploads, then one launch per slots-per-lane class of
// the portfolios inside one timed span (backtest_replay.hip).  The buffers live on the handle (ReplayWs, tangency_host.h).
#include <cstring>
#include <algorithm>
#include <map>
#include <tuple>
#include <vector>

#include "tangency_host.h"

using namespace tp_host;

static_assert(TP_REPLAY_SUM_CHECK == TP_REPLAY_KSTATUS_SUM_CHECK, "replay status codes out of sync");

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
    ReplayWs& ws = h->replay;
    // ---- checks: nothing below them reads outside a caller's array, on the host or on the device
    if (D < 1 || D > 0x7fffffffLL) return fail(h, TP_ERR_INVALID, "tp_replay_run: D=%lld outside [1, 2^31)", (long long)D);
    if (R < 1 || R > D) return fail(h, TP_ERR_INVALID, "tp_replay_run: R=%lld outside [1, D=%lld]", (long long)R, (long long)D);
    if (P < 0 || P > 0x7fffffffLL) return fail(h, TP_ERR_INVALID, "tp_replay_run: P=%lld outside [0, 2^31)", (long long)P);
    if (ld < 1 || K < 1 || K > ld) return fail(h, TP_ERR_INVALID, "tp_replay_run: ld=%d, K=%d: 1 <= K <= ld expected", ld, K);
    if (weights_len < 0 || universe_len < 0) return fail(h, TP_ERR_INVALID, "tp_replay_run: a negative buffer length");
    if (!S || !rf_daily || !reb_day) return fail(h, TP_ERR_INVALID, "tp_replay_run: S, rf_daily or reb_day is NULL");
    if (P > 0 && (!k || !scaling || !cost || !w_off || !w_stride || !u_off || !u_stride || !weights || !cols || !caps))
        return fail(h, TP_ERR_INVALID, "tp_replay_run: a per-portfolio array or a flat buffer is NULL");
    if (reb_day[0] != 0) return fail(h, TP_ERR_INVALID, "tp_replay_run: reb_day[0]=%d, the first trading day rebalances", reb_day[0]);
    for (int64_t j = 1; j < R; ++j)
        if (reb_day[j] <= reb_day[j - 1] || reb_day[j] >= D)
            return fail(h, TP_ERR_INVALID, "tp_replay_run: reb_day[%lld]=%d is not strictly increasing below D=%lld", (long long)j,
                        reb_day[j], (long long)D);
    for (int64_t p = 0; p < P; ++p) {
        if (k[p] < 1) return fail(h, TP_ERR_INVALID, "tp_replay_run: k[%lld]=%d < 1", (long long)p, k[p]);
        if (k[p] > tp_max_assets())
            return fail(h, TP_ERR_UNSUPPORTED, "tp_replay_run: k[%lld]=%d exceeds the largest supported universe %d", (long long)p,
                        k[p], tp_max_assets());
        if (!rows_fit(w_off[p], w_stride[p], R, k[p], weights_len))
            return fail(h, TP_ERR_INVALID, "tp_replay_run: portfolio %lld: w_off=%lld, w_stride=%lld run past the %lld weights",
                        (long long)p, (long long)w_off[p], (long long)w_stride[p], (long long)weights_len);
        if (!rows_fit(u_off[p], u_stride[p], R, k[p], universe_len))
            return fail(h, TP_ERR_INVALID, "tp_replay_run: portfolio %lld: u_off=%lld, u_stride=%lld run past the %lld universe entries",
                        (long long)p, (long long)u_off[p], (long long)u_stride[p], (long long)universe_len);
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
        port[(size_t)p] = tp_replay_port_t{w_off[p], w_stride[p], u_off[p], u_stride[p], it->second, scaling[p], cost[p], k[p], 0};
    }
    std::vector<int32_t> order((size_t)P);
    for (int64_t p = 0; p < P; ++p) order[(size_t)p] = (int32_t)p;
    std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) {
        return tp_replay_slots_per_lane(k[x]) < tp_replay_slots_per_lane(k[y]);
    });
    // ---- device: drain what was queued (the buffers may be in use, the span unread), upload, launch
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    int rc = harvest_kernel_time(h);
    if (rc != TP_OK) return rc;
    ws.ran = false;
    struct Up { DevBuf* b; const void* src; size_t bytes; const char* what; };
    const size_t flat = P > 0 ? 1 : 0;                    // (no portfolio: the flat buffers may be absent)
    const Up ups[] = {
        {&ws.S, S, (size_t)D * (size_t)ld * sizeof(double), "replay returns"},
        {&ws.rf, rf_daily, (size_t)D * sizeof(double), "replay risk-free rates"},
        {&ws.reb, reb_day, (size_t)R * sizeof(int32_t), "replay rebalancing days"},
        {&ws.weights, weights, flat * (size_t)weights_len * sizeof(double), "replay weights"},
        {&ws.cols, cols, flat * (size_t)universe_len * sizeof(int32_t), "replay universes"},
        {&ws.caps, caps, flat * (size_t)universe_len * sizeof(double), "replay market caps"},
        {&ws.prev, prev.data(), prev.size() * sizeof(int32_t), "replay merge maps"},
        {&ws.next, next.data(), next.size() * sizeof(int32_t), "replay merge maps"},
        {&ws.port, port.data(), port.size() * sizeof(tp_replay_port_t), "replay portfolios"},
        {&ws.order, order.data(), order.size() * sizeof(int32_t), "replay launch order"},
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
    ws.ran = true;
    return TP_OK;
}

int tp_replay_download(tp_handle_t h, double* returns, double* turnover, double* metrics, int32_t* status, int32_t* bad_day) {
    if (!h) return TP_ERR_INVALID;
    const ReplayWs& ws = h->replay;
    if (!ws.ran) return fail(h, TP_ERR_INVALID, "tp_replay_download without a tp_replay_run before it");
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t P = (size_t)ws.P, D = (size_t)ws.D, R = (size_t)ws.R;
    return download(h, {{returns, ws.ret.p, P * D * sizeof(double)},
                        {turnover, ws.turnover.p, P * R * sizeof(double)},
                        {metrics, ws.metrics.p, P * R * TP_REPLAY_METRICS * sizeof(double)},
                        {status, ws.status.p, P * sizeof(int32_t)},
                        {bad_day, ws.bad_day.p, P * sizeof(int32_t)}});
}

}  // extern "C"
