// The integer loop's list views: building one beside a freshly compacted working view, and the launches that score it.
// Part of the one translation unit utmos_hip.hip (included there, in order); not a stand-alone header.
//
// A compaction pass drops the variants that are covered for everybody; what a column still streams afterwards is mostly
// cells that are zero for this sample.  A list view keeps, per tile of the view's variant axis and per listed column, the
// positions of the set bits (list.hip.h): an iteration then reads 4 bytes per carrier instead of one bit per variant.  It is
// built only from a view a pass has just written at this batch boundary -- the view's covered mask is empty and the pending
// winner's column is zero in it -- and lives exactly as long as that view: the bitmap view stays resident beside it (the
// pending winner's column and k_view_keep read it), the scoring launches keep the view's covered mask up to date, so a list
// may be dropped at any ABI boundary.  Counts, winners and new_count are the bitmap launches' bit for bit.
#pragma once

static bool any_list(const utm_ctx *c)
{
    for (auto &ch : c->chunks)
        if (ch.lv.valid) return true;
    return false;
}

// A build that does not fit, or that the tile grid cannot count: the chunk keeps its bitmap view for this run.
static void refuse_list(utm_ctx *c, Chunk &ch)
{
    ch.lv.refused = true;
    c->list_refused += 1;
}

// The list view of `ch`'s working view, which a compaction pass has just written: count, scan on the host, fill.
static int build_list(utm_ctx *c, Chunk &ch)
{
    ListView &lv = ch.lv;
    const WorkView &v = ch.work;
    const unsigned n_list = std::min(c->active_ub, c->n_local);  // (v.list: the pass's copy of act[], the columns it moved)
    if (!n_list) return UTM_OK;
    const int t = list_tile_log2(v.wp, c->list_test_t, UTM_LOOP_MAX_TILES_INT);
    if (!t) {
        refuse_list(c, ch);
        return UTM_OK;
    }
    const unsigned tile_words = (1u << t) / 64;
    const u64 tiles = list_tiles(v.wp, t);
    const u64 tab = tiles * c->n_local;
    HIP_TRY(hipEventRecord(c->ev_cmp0, c->stream));
    if (lv.tab_cap < tab + 1) {
        (void)hipFree(lv.counts);
        (void)hipFree(lv.offs);
        lv.counts = lv.offs = nullptr;
        lv.tab_cap = 0;
        HIP_TRY(hipMalloc(&lv.counts, (tab + 1) * 4));
        HIP_TRY(hipMalloc(&lv.offs, (tab + 1) * 4));
        lv.tab_cap = tab + 1;
    }
    const dim3 grid((unsigned)tiles, (unsigned)std::min<u64>(65535, (n_list + 3) / 4));
    HIP_TRY(hipMemsetAsync(lv.counts, 0, tab * 4, c->stream));
    hipLaunchKernelGGL(k_list_count, grid, dim3(256), 0, c->stream, (const u64 *)v.cols, v.wp, tile_words, (const unsigned *)v.list, n_list,
                       c->n_local, lv.counts);
    HIP_TRY(hipGetLastError());
    std::vector<uint32_t> h_counts(tab), h_offs(tab + 1);
    HIP_TRY(copy_sync(c, h_counts.data(), lv.counts, tab * 4, hipMemcpyDeviceToHost));
    lv.col_quads.assign(c->n_local, 0);
    uint64_t n_entries = 0, quads = 0;
    bool ok = list_scan(h_counts.data(), tab, c->n_local, h_offs.data(), lv.col_quads.data(), &n_entries, &quads);
    if (ok && c->list_test_cap && quads * 4 > c->list_test_cap) ok = false;
    if (ok && lv.cap_quads < quads) {
        // (the first build of a context, or of a denser run than any before: later builds of a run are never larger)
        (void)hipFree(lv.entries);
        lv.entries = nullptr;
        lv.cap_quads = 0;
        size_t free_b = 0, total_b = 0;
        HIP_TRY(hipMemGetInfo(&free_b, &total_b));
        const size_t bytes = (size_t)quads * 16 + 64;
        if (bytes > free_b / 2 || hipMalloc(&lv.entries, bytes) != hipSuccess) {
            (void)hipGetLastError();
            lv.entries = nullptr;
            ok = false;
        } else {
            lv.cap_quads = quads;
        }
    }
    i64 bytes = (i64)((u64)n_list * v.w * 8 + tab * 8);  // the listed columns read, the counts cleared and read back
    if (ok) {
        HIP_TRY(hipMemcpyAsync(lv.offs, h_offs.data(), (tab + 1) * 4, hipMemcpyHostToDevice, c->stream));
        if (quads)
            hipLaunchKernelGGL(k_list_fill, grid, dim3(256), 0, c->stream, (const u64 *)v.cols, v.wp, tile_words, (const unsigned *)v.list, n_list,
                               c->n_local, (const unsigned *)lv.offs, lv.entries);
        HIP_TRY(hipGetLastError());
        bytes += (i64)((u64)n_list * v.w * 8 + (tab + 1) * 4 + (u64)n_list * tiles * 8 + quads * 16);  // columns again, offsets, entries out
    }
    HIP_TRY(hipEventRecord(c->ev_cmp1, c->stream));
    HIP_TRY(hipEventSynchronize(c->ev_cmp1));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, c->ev_cmp0, c->ev_cmp1));
    c->list_ms += ms;
    c->list_bytes += bytes;
    c->algo_bytes += bytes;
    if (c->flags & UTM_FLAG_PROFILE_EVENTS) c->score_ms += ms;
    if (!ok) {
        refuse_list(c, ch);
        return UTM_OK;
    }
    lv.valid = lv.had = true;
    lv.t = t;
    lv.n_tiles = (unsigned)tiles;
    lv.sel_quads = quads;
    lv.lanes = list_lanes_of_tile(t, c->list_shape_lanes ? c->list_shape_lanes : list_lanes(quads, tiles, n_list));
    const i64 k = c->list_builds;
    lv.log_slot = k < UTM_LIST_LOG ? (int)k : -1;
    if (k < UTM_LIST_LOG) {
        c->list_log_lanes[k] = lv.lanes;
        c->list_log_wgs[k] = 0;  // (its first launch writes it: launch_score_list)
        c->list_log_iter[k] = c->iter;
        c->list_log_tiles[k] = (int)tiles;
        c->list_log_t[k] = t;
        c->list_log_entries[k] = n_entries;
        c->list_log_padded[k] = quads * 4;
        c->list_log_ms[k] = ms;
        c->list_log_bytes[k] = bytes;
    }
    c->list_builds += 1;
    return UTM_OK;
}

// A compaction pass has just written `ch`'s view: the list of the view before it is gone; build the new view's if the
// policy says so.  (The mailbox form of the fused pick never meets a view: compact_eligible.)
static int list_after_pass(utm_ctx *c, Chunk &ch)
{
    ch.lv.valid = false;
    if (!c->list_on || ch.lv.refused || !ch.work.valid) return UTM_OK;
    const u64 a = std::min(c->active_ub, c->n_local);
    if (!list_policy(c->last_new, ch.work.wp, a, c->list_min_stream, c->list_ratio, ch.lv.had)) return UTM_OK;
    return build_list(c, ch);
}

// Algorithmic bytes of one list-phase iteration of `ch`: the selectable samples' padded entries, their table entries,
// the mask read and written and the winner's words (as the bitmap launches count them).
static i64 list_iteration_bytes(const Chunk &ch, u64 a)
{
    return (i64)(ch.lv.sel_quads * 16 + a * ch.lv.n_tiles * 8 + 3 * score_view(ch).w * 8);
}
// The sample `loc` has been selected: its segments are read no more.
static void list_winner_leaves(utm_ctx *c, i64 loc)
{
    for (auto &ch : c->chunks) {
        ListView &lv = ch.lv;
        if (!lv.valid || loc < 0 || (u64)loc >= lv.col_quads.size()) continue;
        lv.sel_quads -= std::min<u64>(lv.sel_quads, lv.col_quads[(size_t)loc]);
        lv.col_quads[(size_t)loc] = 0;
    }
}

extern "C" int utm_set_list_mode(utm_ctx *c, int32_t mode, uint64_t min_stream_bytes, double ratio)
{
    CTX(c);
    if (mode != 0 && mode != 1) return fail(UTM_EINVAL, "mode %d is neither 0 (off) nor 1 (on)", mode);
    if (ratio < 0) return fail(UTM_EINVAL, "ratio %g is negative", ratio);
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (auto &ch : c->chunks) ch.lv.valid = false;  // (the views' masks are current: the bitmap launches go on from them)
    c->list_on = mode == 1;
    c->list_min_stream = min_stream_bytes ? min_stream_bytes : UTM_LIST_MIN_STREAM_BYTES;
    c->list_ratio = ratio > 0 ? ratio : UTM_LIST_RATIO;
    return UTM_OK;
}

extern "C" int utm_set_list_test(utm_ctx *c, int32_t tile_log2, uint64_t max_entries)
{
    CTX(c);
    if (tile_log2 != 0 && tile_log2 != UTM_LIST_T_TEST && tile_log2 != 16 && tile_log2 != 18 && tile_log2 != 20)
        return fail(UTM_EINVAL, "tile_log2 %d: 0 (the rule), %d, 16, 18 or 20", tile_log2, UTM_LIST_T_TEST);
    c->list_test_t = tile_log2;
    c->list_test_cap = max_entries;
    return UTM_OK;
}

extern "C" int utm_set_list_shape(utm_ctx *c, int32_t lanes, int32_t target_wgs)
{
    CTX(c);
    if (lanes != 0 && lanes != 16 && lanes != 64) return fail(UTM_EINVAL, "lanes %d: 0 (the rule), 16 or 64", lanes);
    if (target_wgs < 0 || target_wgs > UTM_LIST_TARGET_WGS_MAX)
        return fail(UTM_EINVAL, "target_wgs %d: 0 (the rule) or 1 .. %d", target_wgs, UTM_LIST_TARGET_WGS_MAX);
    c->list_shape_lanes = lanes;                    // (from the next build: a list in use keeps the form it was built for)
    c->list_shape_target = (unsigned)target_wgs;    // (from the next launch)
    return UTM_OK;
}

extern "C" int utm_get_list_shape(utm_ctx *c, int32_t *lanes, int32_t *wgs, int32_t *n)
{
    CTX(c);
    if (!lanes || !wgs || !n) return fail(UTM_EINVAL, "an output pointer is NULL");
    *n = (int32_t)std::min<i64>(UTM_LIST_LOG, c->list_builds);
    for (int k = 0; k < UTM_LIST_LOG; ++k) {
        lanes[k] = k < *n ? c->list_log_lanes[k] : 0;
        wgs[k] = k < *n ? c->list_log_wgs[k] : 0;
    }
    return UTM_OK;
}

static_assert(sizeof(((utm_list_stats *)nullptr)->log_iter) / sizeof(int64_t) == UTM_LIST_LOG, "utm_list_stats logs UTM_LIST_LOG builds");
extern "C" int utm_get_list_stats(utm_ctx *c, utm_list_stats *out)
{
    CTX(c);
    if (!out) return fail(UTM_EINVAL, "out is NULL");
    memset(out, 0, sizeof *out);
    out->builds = c->list_builds;
    out->refused = c->list_refused;
    out->build_bytes = c->list_bytes;
    out->build_ms = c->list_ms;
    out->mode = c->list_on ? 1 : 0;
    for (auto &ch : c->chunks) out->valid += ch.lv.valid ? 1 : 0;
    out->min_stream_bytes = c->list_min_stream;
    out->ratio = c->list_ratio;
    for (int k = 0; k < UTM_LIST_LOG && k < c->list_builds; ++k) {
        out->log_iter[k] = c->list_log_iter[k];
        out->log_tiles[k] = c->list_log_tiles[k];
        out->log_t[k] = c->list_log_t[k];
        out->log_entries[k] = c->list_log_entries[k];
        out->log_padded[k] = c->list_log_padded[k];
        out->log_ms[k] = c->list_log_ms[k];
        out->log_bytes[k] = c->list_log_bytes[k];
    }
    return UTM_OK;
}
