// tangency_plan.cpp - host layer of libtangency.so: validation of the caller's inputs, upload planning (which shared
// sums a batch qualifies for) and launch planning of the large-k path (workspace, per-sub-batch tables).
#include <cmath>
#include <cstring>

#include "tangency_host.h"

namespace tp_host {

// Host-side validation of every index the kernel will dereference: a bad offset must never reach
// the device (an out-of-bounds access can take the whole node down).
// price front-end: every (numerator, denominator) row must lie inside the price panel
int validate_pairs(tp_handle_t h, const char* what, const int32_t* num, const int32_t* den, int64_t n, int64_t price_rows) {
    if (!num) return TP_OK;
    if (!den) return fail(h, TP_ERR_INVALID, "%s_num without %s_den", what, what);
    if (n < 1 || n > 0x7fffffffLL) return fail(h, TP_ERR_INVALID, "%s_rows=%lld out of range", what, (long long)n);
    for (int64_t i = 0; i < n; ++i)
        if (num[i] < 0 || num[i] >= price_rows || den[i] < 0 || den[i] >= price_rows)
            return fail(h, TP_ERR_INVALID, "%s pair %lld = (%d, %d) outside the price panel (%lld rows)", what,
                        (long long)i, num[i], den[i], (long long)price_rows);
    return TP_OK;
}

int validate_inputs(tp_handle_t h, const tp_params_t& p, int64_t W, const tp_inputs_t* in_raw) {
    if (!in_raw) return fail(h, TP_ERR_INVALID, "inputs is NULL");
    if (!in_raw->panel || in_raw->panel_rows < 1 || in_raw->panel_ld < 1) return fail(h, TP_ERR_INVALID, "panel missing");
    int rcp = validate_pairs(h, "ret", in_raw->ret_num, in_raw->ret_den, in_raw->ret_rows, in_raw->panel_rows);
    if (rcp != TP_OK) return rcp;
    if (p.strategy == TP_STRATEGY_CONJUGATE && in_raw->hf_panel) {
        rcp = validate_pairs(h, "hf_ret", in_raw->hf_ret_num, in_raw->hf_ret_den, in_raw->hf_ret_rows, in_raw->hf_rows);
        if (rcp != TP_OK) return rcp;
    }
    // with the price front-end the windows address rows of the RETURN panel
    tp_inputs_t eff = *in_raw;
    if (eff.ret_num) eff.panel_rows = eff.ret_rows;
    if (eff.hf_ret_num) eff.hf_rows = eff.hf_ret_rows;
    const tp_inputs_t* in = &eff;
    if (!in->start && !in->row_idx) return fail(h, TP_ERR_INVALID, "need start[] or row_idx[]");
    const bool conj = p.strategy == TP_STRATEGY_CONJUGATE;
    if (conj) {
        if (!in->hf_panel || in->hf_rows < 1 || in->hf_ld < 1) return fail(h, TP_ERR_INVALID, "hf_panel missing");
        if (!in->hf_start && !in->hf_row_idx) return fail(h, TP_ERR_INVALID, "need hf_start[] or hf_row_idx[]");
        if (!in->w0 || !in->n0) return fail(h, TP_ERR_INVALID, "conjugate prior needs w0[] and n0[]");
    }
    const int ncol_need = in->col_idx ? 0 : p.k;
    if (ncol_need > in->panel_ld) return fail(h, TP_ERR_INVALID, "panel_ld=%d < k=%d", in->panel_ld, p.k);
    if (conj && ncol_need > in->hf_ld) return fail(h, TP_ERR_INVALID, "hf_ld=%d < k=%d", in->hf_ld, p.k);
    for (int64_t w = 0; w < W; ++w) {
        const int nr = in->n_rows ? in->n_rows[w] : p.n_r;
        if (nr < 1 || nr > p.n_r) return fail(h, TP_ERR_INVALID, "n_rows[%lld]=%d outside [1,%d]", (long long)w, nr, p.n_r);
        if (in->row_idx) {
            for (int r = 0; r < nr; ++r) {
                const int64_t row = in->row_idx[w * (int64_t)p.n_r + r];
                if (row < 0 || row >= in->panel_rows)
                    return fail(h, TP_ERR_INVALID, "row_idx[%lld][%d]=%lld outside the panel", (long long)w, r, (long long)row);
            }
        } else if (nr > in->panel_rows || in->start[w] < 0 || in->start[w] > in->panel_rows - nr) {   // no start + nr: it may overflow
            return fail(h, TP_ERR_INVALID, "window %lld: %d rows from row %lld lie outside the panel (%lld rows)", (long long)w,
                        nr, (long long)in->start[w], (long long)in->panel_rows);
        }
        if (in->col_idx) {
            for (int j = 0; j < p.k; ++j) {
                const int c = in->col_idx[w * (int64_t)p.k + j];
                if (c < 0 || c >= in->panel_ld || (conj && c >= in->hf_ld))
                    return fail(h, TP_ERR_INVALID, "col_idx[%lld][%d]=%d outside the panel", (long long)w, j, c);
            }
        }
        if (conj) {
            const int mm = in->hf_count ? in->hf_count[w] : p.m;
            if (mm < 2 || mm > p.m) return fail(h, TP_ERR_INVALID, "hf_count[%lld]=%d outside [2,%d]", (long long)w, mm, p.m);
            if (in->hf_row_idx) {
                for (int r = 0; r < mm; ++r) {
                    const int64_t row = in->hf_row_idx[w * (int64_t)p.m + r];
                    if (row < 0 || row >= in->hf_rows)
                        return fail(h, TP_ERR_INVALID, "hf_row_idx[%lld][%d]=%lld outside the panel", (long long)w, r, (long long)row);
                }
            } else if (mm > in->hf_rows || in->hf_start[w] < 0 || in->hf_start[w] > in->hf_rows - mm) {
                return fail(h, TP_ERR_INVALID, "window %lld: %d intraday rows from row %lld lie outside the panel (%lld rows)",
                            (long long)w, mm, (long long)in->hf_start[w], (long long)in->hf_rows);
            }
        }
    }
    return TP_OK;
}

// The arena budget of the large-k path, in entries of `per_entry` bytes: 32 GiB of the 288 (fewer, larger launches: measured
// +2-4 % over 6 GiB at k = 500), never more than a third of what is free (`held`: bytes the caller is about to reallocate,
// counted as free); tiled_arena_gib / tiled_arena_mib override it.
int64_t tiled_arena_entries(tp_handle_t h, size_t per_entry, size_t held) {
    unsigned long long gib = 32;
    { size_t free_b = 0, total_b = 0;
      if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
          free_b += held;
          if ((free_b >> 30) / 3 < gib) gib = (free_b >> 30) / 3 > 1 ? (free_b >> 30) / 3 : 1;
      } }
    if (h->tiled_arena_gib >= 1 && h->tiled_arena_gib <= 200) gib = (unsigned long long)h->tiled_arena_gib;
    unsigned long long arena_bytes = gib << 30;
    if (h->tiled_arena_mib >= 1 && h->tiled_arena_mib <= 200 * 1024) arena_bytes = (unsigned long long)h->tiled_arena_mib << 20;
    int64_t G = (int64_t)(arena_bytes / per_entry);
    if (G < 1) G = 1;
    if (G > 65535) G = 65535;
    return G;
}

// Workspace of the large-k path: ONE arena that holds as many in-flight windows as 32 GiB allow (fewer, larger launches);
// a batch of more windows runs as sub-batches, one after the other on the kernel stream.  (Several small sub-batches in
// flight on streams of their own, their arenas inside the 256 MiB Infinity Cache, measured slower everywhere: DESIGN.md 5.)
int ensure_tiled_ws(tp_batch_t b, tp_tiled_ws_t* ws, int64_t entries) {
    tp_handle_t h = b->h;
    int KP, NS, NSB;
    tp_tiled_geometry(b->p.k, &KP, &NS, &NSB);
    const size_t per_window = sizeof(double) * ((size_t)KP * KP + (size_t)NSB * 64 * 64 + KP + (size_t)b->p.m + 8) + 4;
    int64_t G = tiled_arena_entries(h, per_window);
    if (G > (entries > b->W ? entries : b->W)) G = entries > b->W ? entries : b->W;
    if (b->tiled_capacity < G) {
        int rc = ensure(h, b->t_arena, sizeof(double) * (size_t)G * KP * KP, "large-k arena");
        if (rc == TP_OK) rc = ensure(h, b->t_rinv, sizeof(double) * (size_t)G * NSB * 64 * 64, "large-k inverse diagonal blocks");
        if (rc == TP_OK) rc = ensure(h, b->t_ybar, sizeof(double) * (size_t)G * KP, "large-k column means");
        if (rc == TP_OK) rc = ensure(h, b->t_zc, sizeof(double) * (size_t)G * (b->p.m > 0 ? b->p.m : 1), "large-k intraday scratch");
        if (rc == TP_OK) rc = ensure(h, b->t_scal, sizeof(double) * (size_t)G * 8, "large-k scalars");
        if (rc == TP_OK) rc = ensure(h, b->t_flags, sizeof(int) * (size_t)G, "large-k flags");
        if (rc != TP_OK) return rc;
        b->tiled_capacity = G;
    }
    if (b->hf_B > 0) {
        int rc = ensure(h, b->t_part, sizeof(double) * (size_t)b->tiled_capacity * NS * NS * 64, "large-k prior products");
        if (rc != TP_OK) return rc;
    }
    ws->arena = (double*)b->t_arena.p; ws->rinv = (double*)b->t_rinv.p; ws->ybar = (double*)b->t_ybar.p;
    ws->zc = (double*)b->t_zc.p; ws->scal = (double*)b->t_scal.p; ws->flags = (int*)b->t_flags.p;
    ws->part = (double*)b->t_part.p;
    ws->KP = KP; ws->NS = NS; ws->NSB = NSB;
    return TP_OK;
}

// Shared daily sums of the large-k path for ONE sub-batch: the 16-row blocks its windows cover, block Grams first, one
// table of block-window sums per whole-block count behind them.
int plan_daily_tables(tp_batch_t b, tp_kargs_t& sub) {
    tp_handle_t h = b->h;
    sub.prefix = nullptr; sub.winsum = nullptr; sub.prefix_nblk = 0; sub.prefix_blk0 = 0;
    for (int i = 0; i < 4; ++i) sub.winsum_L[i] = 0;
    long long lo = 0x7fffffffffffffffLL, hi = -1;
    for (int64_t w = sub.w_first; w < sub.w_first + sub.w_count; ++w) {
        const long long f = b->h_start[(size_t)w], cnt = b->h_n_rows.empty() ? b->p.n_r : b->h_n_rows[(size_t)w];
        const long long b0 = (f + 15) / 16, b1 = (f + cnt) / 16;
        if (b1 <= b0) continue;
        if (b0 < lo) lo = b0;
        if (b1 > hi) hi = b1;
    }
    if (hi <= lo) return TP_OK;
    if (hi > b->prefix_nblk) hi = b->prefix_nblk;
    // sharing pays while the windows' rows outnumber the rows of the blocks a few times over
    if ((double)sub.w_count * b->p.n_r < 3.0 * 16.0 * (double)(hi - lo)) return TP_OK;
    const long long nblk = hi - lo;
    int n_L = 0;
    while (n_L < TP_WINSUM_MAX_L && b->winsum_L[n_L] > 0) ++n_L;
    if (nblk < 1 || nblk > 0x3fffffff || n_L == 0) return TP_OK;
    const size_t slot = tp_tiled_slot_doubles(b->p.k);
    const size_t bytes = sizeof(double) * (size_t)nblk * (size_t)(1 + n_L) * slot;
    if (bytes > b->prefix.bytes) {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || bytes > (free_b + b->prefix.bytes) / 3) return TP_OK;
        int rc = ensure(h, b->prefix, bytes, "shared daily block sums");
        if (rc != TP_OK) return rc;
    }
    sub.prefix = (const double*)b->prefix.p;
    sub.winsum = (const double*)b->prefix.p + (size_t)nblk * slot;
    sub.prefix_nblk = (int)nblk;
    sub.prefix_blk0 = (int)lo;
    for (int i = 0; i < 4; ++i) sub.winsum_L[i] = b->winsum_L[i];
    return TP_OK;
}

// Shared intraday sums of ONE sub-batch (windows sub.w_first .. + sub.w_count): the block range its windows cover, the
// tables sized for it (block Grams, then the block-window sums).  A sub-batch whose windows do not all have hf_L whole blocks
// inside one affordable range keeps the two-pass form (sub.hf_winsum stays null).
int plan_hf_tables(tp_batch_t b, tp_kargs_t& sub) {
    tp_handle_t h = b->h;
    sub.hf_prefix = nullptr; sub.hf_winsum = nullptr;
    const long long B = b->hf_B, ph = b->hf_phase, m = b->p.m;
    long long lo = 0x7fffffffffffffffLL, hi = -1;
    for (int64_t w = sub.w_first; w < sub.w_first + sub.w_count; ++w) {
        const long long f = b->h_hf_start[(size_t)w];
        const long long b0 = (f - ph + B - 1) / B, b1 = (f + m - ph) / B;      // f - ph > -B
        if (b1 - b0 != b->hf_L) return TP_OK;
        if (b0 < lo) lo = b0;
        if (b1 > hi) hi = b1;
    }
    // the table starts on a multiple of the block-window sums' group length: a position's sum is then the same sequence of
    // additions whichever sub-batch asks for it (results do not depend on how a run is cut into sub-batches)
    const long long run = b->hf_L < TP_WINSUM_RUN ? b->hf_L : TP_WINSUM_RUN;
    lo = (lo / run) * run;
    const long long nblk = hi - lo;
    if (nblk < b->hf_L || nblk > 0x3fffffff) return TP_OK;
    // sharing pays while the windows outnumber the blocks they touch a few times over
    if ((double)sub.w_count * (double)b->hf_L < 2.0 * (double)nblk) return TP_OK;
    const size_t slot = tp_tiled_slot_doubles(b->p.k);
    const size_t bytes = sizeof(double) * 2 * (size_t)nblk * slot;
    if (bytes > b->hf_prefix.bytes) {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || bytes > (free_b + b->hf_prefix.bytes) / 2) return TP_OK;
        int rc = ensure(h, b->hf_prefix, bytes, "shared intraday block sums");
        if (rc != TP_OK) return rc;
    }
    sub.hf_prefix = (const double*)b->hf_prefix.p;
    sub.hf_winsum = (const double*)b->hf_prefix.p + (size_t)nblk * slot;
    sub.hf_row0 = ph + B * lo;
    sub.hf_blk_rows = (int)B;
    sub.hf_nblk = (int)nblk;
    sub.hf_L = b->hf_L;
    return TP_OK;
}

// Rolling windows over one shared panel overlap almost entirely; the register-tile path then takes the whole aligned
// row blocks of every window from block-window Gram sums of the panel that all windows share (one kernel straight from the
// panel, posterior_shared_tables.hip - or, option shared_tables = 0, block_gram_kernel + tp_window_sums_kernel; the tiled
// path: tiled_block_gram_kernel + tp_window_sums_kernel) instead of pushing every row of every window through the MFMAs.  Qualifies: contiguous windows
// (start[]), no column gather, no per-row risk-free adjustment, k in the register-tile range, and windows that
// together cover the panel at least three times.  The sums are recomputed by EVERY tp_batch_run (nothing is kept
// between runs); TP_FLAG_NO_SHARED_GRAM switches the scheme off.
int plan_shared_gram(tp_batch_t b, const tp_inputs_t* in, hipStream_t st) {
    tp_handle_t h = b->h;
    b->prefix_nblk = 0;
    b->prefix_per_sub = false;
    b->winsum_zero = false;
    b->h_start.clear(); b->h_n_rows.clear();
    const tp_params_t& p = b->p;
    if ((p.flags & TP_FLAG_NO_SHARED_GRAM) || h->no_shared_gram) return TP_OK;
    if (in->row_idx || in->col_idx || in->rf_adj || !in->start) return TP_OK;
    const long long rows = in->ret_num ? in->ret_rows : in->panel_rows;
    int nblk = 0;
    size_t bytes = 0;
    for (int i = 0; i < 4; ++i) b->winsum_L[i] = 0;
    {
        // one table of block-window sums per whole-block count that occurs among the windows (rolling windows of one
        // length have two: 249 rows over 16-row blocks cover 14 or 15 whole blocks)
        const bool fused = p.k <= tp_fused_max_assets();
        const int blk = fused ? TP_PREFIX_BLOCK_ROWS((p.k + 1 + 15) / 16) : 16;
        int n_L = 0;
        for (int64_t w = 0; w < b->W; ++w) {
            const long long first = in->start[w], cnt = in->n_rows ? in->n_rows[w] : p.n_r;
            const long long L = (first + cnt) / blk - (first + blk - 1) / blk;
            if (L < 1) continue;
            int i = 0;
            while (i < n_L && b->winsum_L[i] != (int)L) ++i;
            if (i == n_L) {
                if (n_L == TP_WINSUM_MAX_L) { for (int q = 0; q < 4; ++q) b->winsum_L[q] = 0; return TP_OK; }   // irregular windows: no sharing
                b->winsum_L[n_L++] = (int)L;
            }
        }
        if (n_L == 0) return TP_OK;
        bytes = fused ? tp_fused_prefix_bytes(p.k, rows, n_L, &nblk) : tp_tiled_prefix_bytes(p.k, rows, n_L, &nblk);
    }
    if (nblk < 2 || (double)b->W * p.n_r < 3.0 * (double)rows) return TP_OK;
    // a handful of tiny windows: building the tables costs more than the rows they save (configs[0], k = 10, 100 windows:
    // 28.6 us with the shared sums, 21.5 us without - measured when the tables took two launches; the gate decides which
    // batches share and so what they compute, and stays where it is)
    if (p.k <= 31 && b->W < 256) return TP_OK;
    if (p.k > tp_fused_max_assets()) {
        // large-k path: a slot is megabytes (4.35 MB at k = 1000), a table over the whole panel of a long run does not fit
        // (102 GB at 125,000 windows) - the tables are built per sub-batch, for the blocks its windows cover
        if ((size_t)in->panel_ld * 8 * 4096 >= (1ull << 32)) return TP_OK;
        b->prefix_per_sub = true;
        b->prefix_nblk = nblk;
        b->h_start.assign(in->start, in->start + b->W);
        if (in->n_rows) b->h_n_rows.assign(in->n_rows, in->n_rows + b->W);
        return TP_OK;
    }
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || bytes > free_b / 3) return TP_OK;   // never crowd out the batch itself
    if ((size_t)in->panel_ld * 8 * 4096 >= (1ull << 32)) return TP_OK;      // 32-bit offsets inside a segment
    // One more slot behind the tables, all zero and written by no kernel.  The one-wave kernel's preloaded form starts a
    // window's accumulators from its table slot, and a window without one from this slot.  That form accumulates the
    // intraday rows scaled by sqrt(n0 m / (m - 1)): a batch with a negative or non-finite prior strength, or a window with
    // fewer than two intraday rows, keeps the form that scales afterwards (its statuses are the reference there).
    const size_t slot_bytes = sizeof(double) * tp_fused_slot_doubles(p.k);
    int rc = ensure(h, b->prefix, bytes + slot_bytes, "shared daily block sums");
    if (rc != TP_OK) return rc;
    bool pre = p.strategy == TP_STRATEGY_CONJUGATE && in->n0 != nullptr && !in->hf_row_idx;
    for (int64_t w = 0; pre && w < b->W; ++w) {
        if (!(in->n0[w] >= 0.0) || !std::isfinite(in->n0[w])) pre = false;
        if (in->hf_count && in->hf_count[w] < 2) pre = false;
    }
    if (pre) {
        HIP_TRY(h, hipMemsetAsync((char*)b->prefix.p + bytes, 0, slot_bytes, st));      // on the upload's stream, like its copies
        b->winsum_zero = true;
    }
    b->prefix_nblk = nblk;
    return TP_OK;
}

// Large-k path, conjugate: do the intraday windows qualify for shared sums (posterior_tiled_wave.h)?  Contiguous windows of
// ONE length over ungathered columns, all starts a multiple of a stride B apart (rolling dates: one day of bars),
// a contiguous daily layout without a risk-free adjustment (the kernel variant is built for that), and at least two whole
// B-row blocks per window.  Blocks are aligned to the windows' ENDS: a window that starts behind a day's first bar
// (its return is undefined, ref:311-312) ends on a day boundary.
void plan_shared_hf(tp_batch_t b, const tp_inputs_t* in) {
    tp_handle_t h = b->h;
    const tp_params_t& p = b->p;
    b->hf_B = 0; b->hf_L = 0; b->hf_phase = 0;
    b->h_hf_start.clear();
    if (p.strategy != TP_STRATEGY_CONJUGATE || p.k <= tp_fused_max_assets()) return;
    if ((p.flags & TP_FLAG_NO_SHARED_GRAM) || h->no_shared_gram) return;
    if (!in->hf_start || in->hf_row_idx || in->hf_count || in->col_idx || in->row_idx || in->rf_adj || !in->start) return;
    if (b->W < 4) return;
    // B: the largest stride all starts are multiples of (apart from a common offset) - the order of the windows in the
    // batch does not matter, a reversed or shuffled batch takes the same decision and the same tables
    long long B = 0;
    for (int64_t w = 1; w < b->W; ++w) {
        long long d = in->hf_start[w] - in->hf_start[0];
        if (d < 0) d = -d;
        while (d != 0) { const long long t = B % d; B = d; d = t; }       // B = gcd(B, d)
    }
    if (B < 16 || B > 4096) return;
    const long long m = p.m;
    const long long ph = (in->hf_start[0] + m) % B;      // (start - ph > -B: the ceilings below stay exact)
    const long long f = in->hf_start[0];
    const long long L = (f + m - ph) / B - (f - ph + B - 1) / B;
    // Measured at k = 500 (8,192 windows): with L = 4 whole days per window the tables cost what they save (block Grams 0.52 us +
    // block-window sums 0.43 us + a second slot read per window against 312 rows at 4.6 ns); at k = 1,000 with L = 21:
    // 21.1 k -> 49.3 k windows/s.  Break-even L = 3.5; shared from 6 (option hf_share_min_blocks, tests use 2).
    if (L < 2 || L < h->hf_share_min_blocks) return;
    b->hf_B = (int)B; b->hf_L = (int)L; b->hf_phase = ph;
    b->h_hf_start.assign(in->hf_start, in->hf_start + b->W);
}

}  // namespace tp_host
