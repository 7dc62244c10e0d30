// The integer loop's working views: when to make one, the compaction pass, and how the chunks' own covered masks follow.
// Part of the one translation unit utmos_hip.hip (included there, in order); not a stand-alone header.
//
// An iteration counts popcount(column & ~covered): every covered position is read and then ANDed away, and covered only
// grows.  So at a batch boundary the loop may replace what it scores by a copy of the columns without the covered
// positions (k_filter_compact under keep = ~covered), with an empty covered mask of its own.  Counts, winners and
// new_count are the same bit for bit: a sample's uncovered carriers are the same set, only renumbered, and the samples
// keep their column index.  The chunk's columns and its full-size covered mask stay where they are for everything else;
// while a view is valid the scoring launches update the view's mask only, and k_or_rows brings the chunk's mask up to
// date from the result rows before utm_run returns.  The first copy of a run is made from the chunk's columns, every later
// one from the view before it (two column blocks per chunk, used in turn): nothing outside the loop reads view
// coordinates, so there is no coordinate map to chain.  A pass moves the columns of the samples that are still selectable;
// the zero fill stands for the others, whose columns no scoring launch reads from a view.
#pragma once

// What the integer scoring launches read for a chunk: its working view while that is valid, else the chunk itself.
struct ScoreView {
    const u64 *cols;
    u64 *covered;
    u64 n_var, w, wp;
};
static ScoreView score_view(const Chunk &ch)
{
    if (ch.work.valid) return ScoreView{ch.work.cols, ch.work.covered, ch.work.n_var, ch.work.w, ch.work.wp};
    return ScoreView{ch.cols, ch.covered, ch.n_var, ch.w, ch.wp};
}
// Words per sample of what the integer loop streams (the sum of wp over the chunks' views).
static u64 work_col_words(const utm_ctx *c)
{
    u64 words = 0;
    for (auto &ch : c->chunks) words += score_view(ch).wp;
    return words;
}
static bool any_view(const utm_ctx *c)
{
    for (auto &ch : c->chunks)
        if (ch.work.valid) return true;
    return false;
}

// Views are for the plain integer loop on the only shard: AF tables and chains, depth planes, the decremental copies and
// the peers' mappings all address the chunk's own columns.
static bool compact_eligible(const utm_ctx *c)
{
    return c->compact_on && !c->compact_refused && c->af_mode == UTM_AF_NONE && c->depth == 1 && !c->decr_enabled && c->n_ranks == 1 &&
           c->n_local == c->n_total && !c->comm && !c->p2p && !c->remote_winner_test;
}

// k_filter_compact over every local column, or over the n_list columns of `list` (device memory): about 16k workgroups,
// tiles x column groups, a group at least 8 columns so that a lane's masks are worth deriving.  `out` is zero-filled,
// prefix[w_in] <= 64 wp_out.
static int launch_filter_compact(utm_ctx *c, const u64 *cols, u64 wp, u64 w_in, const u64 *keep, const u64 *prefix, u64 *out, u64 wp_out,
                                 const unsigned *list = nullptr, unsigned n_list = 0)
{
    const unsigned n_cols = list ? n_list : c->n_local;
    if (!n_cols) return UTM_OK;
    const u64 tiles = (wp + UTM_FILTER_TILE_WORDS - 1) / UTM_FILTER_TILE_WORDS;
    if (tiles > 0x7FFFFFFFull) return fail(UTM_EINVAL, "chunk too large for one compaction launch");
    const u64 want_groups = std::max<u64>(1, 16384 / tiles);
    u64 per_group = std::max<u64>({8, (n_cols + want_groups - 1) / want_groups, ((u64)n_cols + 65534) / 65535});
    per_group = round_up(per_group, UTM_FILTER_U);
    const dim3 grid((unsigned)tiles, (unsigned)((n_cols + per_group - 1) / per_group));
    const bool nt = c->tune.nt_loads >= 0 ? c->tune.nt_loads != 0 : (u64)n_cols * wp * 8 > ((u64)c->tune.nt_min_mb << 20);
    if (nt)
        hipLaunchKernelGGL((k_filter_compact<true>), grid, dim3(256), 0, c->stream, cols, wp, w_in, keep, prefix, out, wp_out, n_cols,
                           (unsigned)per_group, list);
    else
        hipLaunchKernelGGL((k_filter_compact<false>), grid, dim3(256), 0, c->stream, cols, wp, w_in, keep, prefix, out, wp_out, n_cols,
                           (unsigned)per_group, list);
    HIP_TRY(hipGetLastError());
    return UTM_OK;
}

// The chunk's own covered mask as of `iter` result rows.  Without a view the scoring launches have kept it up to date but
// for the pending winner; with one, the winners of rows [r0, iter) are missing (the pending one among them): one launch
// over all of them, however many views the chunk has had since.
static int flush_chunk_covered(utm_ctx *c, Chunk &ch)
{
    const unsigned blocks = (unsigned)std::min<u64>(1024, (ch.wp + 255) / 256);
    if (!ch.work.valid) {
        hipLaunchKernelGGL(k_apply_pending, dim3(blocks), dim3(256), 0, c->stream, ch.covered, ch.cols, ch.wp, pending_of(c, ch, false), c->d_st, 0);
    } else if (ch.work.r0 < c->iter) {
        hipLaunchKernelGGL(k_or_rows, dim3(blocks), dim3(256), 0, c->stream, ch.covered, (const u64 *)ch.cols, ch.wp, (const i64 *)c->d_res_idx,
                           ch.work.r0, c->iter, c->first, c->n_local);
        c->compact_bytes += (i64)((u64)(c->iter - ch.work.r0 + 2) * ch.w * 8);
        ch.work.r0 = c->iter;
    }
    HIP_TRY(hipGetLastError());
    return UTM_OK;
}

// Before utm_run returns (and wherever else the chunks' masks are about to be read): every chunk's covered mask current.
static int flush_views(utm_ctx *c)
{
    if (!any_view(c)) return UTM_OK;
    const i64 bytes0 = c->compact_bytes;
    HIP_TRY(hipEventRecord(c->ev_cmp0, c->stream));
    for (auto &ch : c->chunks)
        if (ch.work.valid) TRY(flush_chunk_covered(c, ch));
    HIP_TRY(hipEventRecord(c->ev_cmp1, c->stream));
    HIP_TRY(hipEventSynchronize(c->ev_cmp1));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, c->ev_cmp0, c->ev_cmp1));
    c->compact_ms += ms;
    c->algo_bytes += c->compact_bytes - bytes0;
    if (c->flags & UTM_FLAG_PROFILE_EVENTS) c->score_ms += ms;  // (the roofline stays bytes over time of the same launches)
    return UTM_OK;
}

// The small buffers of a pass: keep words, their prefix counts, the view's covered mask (a view is never longer than its
// chunk), the pass's copy of act[].
static int reserve_view_masks(utm_ctx *c, Chunk &ch)
{
    WorkView &v = ch.work;
    if (!v.keep) HIP_TRY(hipMalloc(&v.keep, ch.wp * 8));
    if (!v.prefix) HIP_TRY(hipMalloc(&v.prefix, (ch.wp + 1) * 8));
    if (!v.covered) HIP_TRY(hipMalloc(&v.covered, ch.wp * 8));
    if (!v.list) HIP_TRY(hipMalloc(&v.list, ((size_t)c->n_local + 1) * 4));
    return UTM_OK;
}

// Column block `b` of the view for a copy of wp_out words per column, or *ok = false: no room.  (Never the block a valid
// view lives in: the first pass of a run has none, a later one asks for the other block.)
static int reserve_view(utm_ctx *c, Chunk &ch, int b, u64 wp_out, bool *ok)
{
    WorkView &v = ch.work;
    *ok = false;
    const u64 need = compact_capacity_words(c->n_local, wp_out);
    if (!need) return UTM_OK;
    if (v.cap_words[b] < need) {
        (void)hipFree(v.blk[b]);
        v.blk[b] = nullptr;
        v.cap_words[b] = 0;
        size_t free_b = 0, total_b = 0;
        HIP_TRY(hipMemGetInfo(&free_b, &total_b));
        const size_t bytes = (size_t)need * 8 + UTM_COLS_SLACK_BYTES;
        if (bytes > free_b / 2) return UTM_OK;
        if (hipMalloc(&v.blk[b], bytes) != hipSuccess) {
            (void)hipGetLastError();
            v.blk[b] = nullptr;
            return UTM_OK;
        }
        v.cap_words[b] = need;
    }
    *ok = true;
    return UTM_OK;
}

// (`left`: the iterations the running utm_run call still wants)
static CompactDecision chunk_policy(const utm_ctx *c, const Chunk &ch, u64 uncovered, i64 left)
{
    const ScoreView sv = score_view(ch);
    return compact_policy(sv.n_var, uncovered, c->compact_min_vars, c->compact_ratio, c->iter, c->active_ub, sv.wp, left);
}

// One chunk at a batch boundary (the device is idle, `iter` rows are out): measure what is left of what the loop scores
// and, if the policy says so, make the view anew -- from the chunk's columns when it has no view, else from the view.
static int compact_chunk(utm_ctx *c, Chunk &ch, i64 left)
{
    WorkView &v = ch.work;
    const bool from_view = v.valid;
    const ScoreView src = score_view(ch);
    const i64 bytes0 = c->compact_bytes;
    HIP_TRY(hipEventRecord(c->ev_cmp0, c->stream));
    TRY(reserve_view_masks(c, ch));
    const unsigned keep_blocks = (unsigned)std::max<u64>(1, std::min<u64>(1024, (src.w + 255) / 256));
    if (!from_view) {
        // the chunk's covered mask with the pending winner, then keep = what it leaves
        TRY(flush_chunk_covered(c, ch));
        hipLaunchKernelGGL(k_compact_keep, dim3(keep_blocks), dim3(256), 0, c->stream, (const u64 *)ch.covered, ch.w, ch.n_var, v.keep);
    } else {
        // keep = what neither the view's mask nor the pending winner's column in the view covers; the chunk's own mask
        // waits for flush_views
        hipLaunchKernelGGL(k_view_keep, dim3(keep_blocks), dim3(256), 0, c->stream, (const u64 *)v.covered, (const u64 *)v.cols, v.wp,
                           pending_of(c, ch, false), (const IterState *)c->d_st, v.w, v.n_var, v.keep);
    }
    hipLaunchKernelGGL(k_filter_prefix, dim3(1), dim3(UTM_FILTER_SCAN_THREADS), 0, c->stream, (const u64 *)v.keep, src.w, v.prefix);
    HIP_TRY(hipGetLastError());
    u64 kept = 0;
    HIP_TRY(copy_sync(c, &kept, v.prefix + src.w, 8, hipMemcpyDeviceToHost));
    c->compact_bytes += (i64)(src.w * 8 * (from_view ? 5 : 4) + 8);  // covered (and the pending column) read, keep written and read, prefix written
    v.known_uncov = kept;
    v.known_tot = c->captured_seen;
    bool done = false;
    if (kept <= src.n_var && chunk_policy(c, ch, kept, left).compact) {
        const u64 wp_out = compact_wp(kept);
        const int dst = from_view ? 1 - v.cur : 0;
        bool ok = false;
        TRY(reserve_view(c, ch, dst, wp_out, &ok));
        if (!ok && from_view) {
            v.stuck = true;  // the chunk keeps the view it has
            c->view_refused += 1;
        } else if (!ok) {
            c->compact_refused = true;
        } else {
            const size_t bytes = (size_t)c->n_local * wp_out * 8 + UTM_COLS_SLACK_BYTES;
            // the columns to move: act[] as the last launch left it (the host is synchronised; every selectable sample is
            // in its first active_ub entries, the pending winner has left it), in a buffer of the pass's own
            const unsigned n_list = std::min(c->active_ub, c->n_local);
            if (n_list) HIP_TRY(hipMemcpyAsync(v.list, c->d_act, (size_t)n_list * 4, hipMemcpyDeviceToDevice, c->stream));
            HIP_TRY(hipMemsetAsync(v.blk[dst], 0, bytes, c->stream));
            if (kept) TRY(launch_filter_compact(c, src.cols, src.wp, src.w, v.keep, v.prefix, v.blk[dst], wp_out, v.list, n_list));
            HIP_TRY(hipMemsetAsync(v.covered, 0, wp_out * 8, c->stream));  // (behind the keep kernel that read it)
            v.cols = v.blk[dst];
            v.cur = dst;
            v.n_var = kept;
            v.w = (kept + 63) / 64;
            v.wp = wp_out;
            if (!from_view) v.r0 = c->iter;
            v.valid = true;
            // the list copied and read, keep and prefix read by the lanes, the listed columns in, the zero fill and the
            // kept words out, the view's mask cleared
            c->compact_bytes += (i64)((u64)n_list * 12 + src.w * 8 * 2 + (u64)n_list * src.w * 8 + bytes + (u64)n_list * v.w * 8 + wp_out * 8);
            done = true;
        }
    }
    HIP_TRY(hipEventRecord(c->ev_cmp1, c->stream));
    HIP_TRY(hipEventSynchronize(c->ev_cmp1));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, c->ev_cmp0, c->ev_cmp1));
    c->compact_ms += ms;
    c->algo_bytes += c->compact_bytes - bytes0;
    if (c->flags & UTM_FLAG_PROFILE_EVENTS) c->score_ms += ms;
    if (done) {
        const i64 k = c->compactions;
        if (k < UTM_COMPACT_LOG) {
            c->compact_pass_iter[k] = c->iter;
            c->compact_pass_vars[k] = kept;
            c->compact_pass_ms[k] = ms;
            c->compact_pass_src[k] = from_view ? 1 : 0;
        }
        c->compactions += 1;
        if (from_view) c->view_passes += 1;
    }
    return UTM_OK;
}

// Every chunk at a batch boundary; *batch = the longest batch the chunks' policies allow next.  A chunk is measured only
// when it may pass its rule: since its last measurement it cannot have lost more variants than the whole matrix has
// captured (exact for one chunk), and both rules -- the caller's share and the library's saving rule -- only get easier
// to pass as `uncovered` falls, so the lower bound decides.
static int list_after_pass(utm_ctx *c, Chunk &ch);  // (host_list.hip.h)
static int compact_at_boundary(utm_ctx *c, int *batch, i64 left)
{
    *batch = UTM_COMPACT_BATCH;
    for (auto &ch : c->chunks) {
        if (c->compact_refused) break;
        if (ch.work.stuck) continue;
        const u64 gone = (u64)std::max<i64>(0, c->captured_seen - ch.work.known_tot);
        const u64 at_least = ch.work.known_uncov > gone ? ch.work.known_uncov - gone : 0;
        const i64 passes0 = c->compactions;
        if (chunk_policy(c, ch, at_least, left).compact) TRY(compact_chunk(c, ch, left));
        if (c->compactions != passes0) TRY(list_after_pass(c, ch));  // (a new view: the list of the one before is gone)
        if (ch.work.stuck) continue;
        *batch = std::min(*batch, chunk_policy(c, ch, ch.work.known_uncov, left).batch);
    }
    return UTM_OK;
}

extern "C" int utm_set_compaction(utm_ctx *c, int32_t mode, uint64_t min_vars, double ratio)
{
    CTX(c);
    if (mode != 0 && mode != 1) return fail(UTM_EINVAL, "mode %d is neither 0 (off) nor 1 (on)", mode);
    if (ratio >= 1.0) return fail(UTM_EINVAL, "ratio %g: a copy must drop something (below 1)", ratio);
    HIP_TRY(hipStreamSynchronize(c->stream));
    invalidate_views(c);  // (the chunks' masks are current: utm_run left them so)
    c->compact_on = mode == 1;
    // (both left at 0: the library's policy by cost; one of them given: the other takes its explicit-form default)
    const bool by_cost = !min_vars && !(ratio > 0);
    c->compact_min_vars = by_cost ? 0 : min_vars ? min_vars : UTM_COMPACT_MIN_VARS;
    c->compact_ratio = by_cost ? 0.0 : ratio > 0 ? ratio : UTM_COMPACT_RATIO;
    return UTM_OK;
}

static_assert(sizeof(((utm_compaction_stats *)nullptr)->log_iter) / sizeof(int64_t) == UTM_COMPACT_LOG, "utm_compaction_stats logs UTM_COMPACT_LOG passes");
extern "C" int utm_get_compaction_stats(utm_ctx *c, utm_compaction_stats *out)
{
    CTX(c);
    if (!out) return fail(UTM_EINVAL, "out is NULL");
    memset(out, 0, sizeof *out);
    out->compactions = c->compactions;
    for (auto &ch : c->chunks) out->working_vars += score_view(ch).n_var;
    out->pass_bytes = c->compact_bytes;
    out->pass_ms = c->compact_ms;
    out->refused = c->compact_refused ? 1 : 0;
    out->mode = c->compact_on ? 1 : 0;
    out->min_vars = c->compact_min_vars;
    out->ratio = c->compact_ratio;
    out->view_passes = c->view_passes;
    out->view_refused = c->view_refused;
    out->stream_bytes = UTM_COMPACT_STREAM_BYTES;
    out->pass_cost = UTM_COMPACT_PASS_COST;
    for (int k = 0; k < UTM_COMPACT_LOG && k < c->compactions; ++k) {
        out->log_iter[k] = c->compact_pass_iter[k];
        out->log_vars[k] = c->compact_pass_vars[k];
        out->log_ms[k] = c->compact_pass_ms[k];
        out->log_src[k] = c->compact_pass_src[k];
    }
    return UTM_OK;
}
