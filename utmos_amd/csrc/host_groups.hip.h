// Group curves: utm_group_curve (k_group_unions + k_group_curve over one chunk) and the CPU build of the same arithmetic.
// Part of the one translation unit utmos_hip.hip (included there, in order); not a stand-alone header.
#pragma once

// The samples with a group id, sorted by group (a counting sort: inside a group by index), and the G + 1 offsets.
static int group_sort(const int32_t *group_of, u64 n_samp, i64 n_groups, std::vector<unsigned> *sorted, std::vector<unsigned> *offs)
{
    if (!group_of) return fail(UTM_EINVAL, "group_of is NULL");
    if (n_groups < 1 || n_groups > UTM_GROUPS_MAX) return fail(UTM_EINVAL, "%lld groups not in 1..%d", (long long)n_groups, UTM_GROUPS_MAX);
    offs->assign((size_t)n_groups + 1, 0u);
    for (u64 s = 0; s < n_samp; ++s) {
        const i64 g = group_of[s];
        if (g < -1 || g >= n_groups) return fail(UTM_EINVAL, "sample %llu: group %lld not in -1..%lld", (unsigned long long)s, (long long)g, (long long)n_groups - 1);
        if (g >= 0) ++(*offs)[(size_t)g + 1];
    }
    for (i64 g = 0; g < n_groups; ++g) (*offs)[(size_t)g + 1] += (*offs)[(size_t)g];
    sorted->resize((*offs)[(size_t)n_groups]);
    std::vector<unsigned> at(offs->begin(), offs->end() - 1);
    for (u64 s = 0; s < n_samp; ++s)
        if (group_of[s] >= 0) (*sorted)[at[(size_t)group_of[s]]++] = (unsigned)s;
    return UTM_OK;
}

extern "C" int utm_group_curve(utm_ctx *c, int32_t chunk, const int32_t *group_of, int32_t n_groups, const int64_t *global_idx, int64_t n,
                               uint32_t bin_mode, int64_t *new_out, int64_t *priv_out, int64_t *total_out, int64_t *ptotal_out, double *pass_ms)
{
    CTX(c);
    if (!group_of || !total_out || n < 0 || (n > 0 && (!global_idx || !new_out))) return fail(UTM_EINVAL, "bad arguments");
    if (bin_mode > 2) return fail(UTM_EINVAL, "bin_mode %u not in 0..2", bin_mode);
    Chunk *ch;
    TRY(chunk_of(c, chunk, &ch));
    if (depth_sharded(c))
        return fail(UTM_ESTATE, "group curves need the whole sample axis in one context without an exchange (this one holds samples "
                                "%u..%u of %u)", c->first, c->first + c->n_local, c->n_total);
    if (n > (i64)c->n_total || n > (i64)INT32_MAX) return fail(UTM_EINVAL, "%lld samples listed, the matrix has %u", (long long)n, c->n_total);
    std::vector<unsigned> sorted, offs, order;
    TRY(group_sort(group_of, c->n_total, n_groups, &sorted, &offs));
    TRY(pair_list(global_idx, (u64)n, c->n_total, "order", &order));
    const unsigned G = (unsigned)n_groups;
    const bool priv = priv_out != nullptr;
    const unsigned rows = priv ? 2 * G : G;
    const size_t cells = (size_t)rows * (size_t)n;
    if (pass_ms) *pass_ms = 0.0;
    if (ch->n_var == 0) {
        std::fill(total_out, total_out + G, (int64_t)0);
        if (ptotal_out) std::fill(ptotal_out, ptotal_out + G, (int64_t)0);
        if (n) std::fill(new_out, new_out + (size_t)G * (size_t)n, (int64_t)0);
        if (n && priv) std::fill(priv_out, priv_out + (size_t)G * (size_t)n, (int64_t)0);
        return UTM_OK;
    }

    // Nothing of the context is read but the chunk's columns, and nothing of it is written: the lists, the masks, the bins
    // and the events are this call's own.  The launches go on the context's stream, behind whatever wrote the columns.
    Scratch<unsigned> d_sorted, d_offs, d_order;
    Scratch<u64> d_masks, d_totals, d_bins;
    HIP_TRY(d_masks.alloc((size_t)(G + 1) * (size_t)ch->wp));  // (UTM_ENOMEM when it cannot be had)
    HIP_TRY(d_sorted.alloc(std::max<size_t>(sorted.size(), 1)));
    HIP_TRY(d_offs.alloc((size_t)G + 1));
    HIP_TRY(d_totals.alloc((size_t)2 * G));
    if (!sorted.empty()) HIP_TRY(hipMemcpyAsync(d_sorted.p, sorted.data(), sorted.size() * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(d_offs.p, offs.data(), ((size_t)G + 1) * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(d_totals.p, 0, (size_t)2 * G * 8, c->stream));
    if (n) {
        HIP_TRY(d_order.alloc((size_t)n));
        HIP_TRY(d_bins.alloc(cells));
        HIP_TRY(hipMemcpyAsync(d_order.p, order.data(), (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemsetAsync(d_bins.p, 0, cells * 8, c->stream));
    }
    struct Events {
        hipEvent_t e0 = nullptr, e1 = nullptr;
        ~Events() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
    } ev;
    if (pass_ms) {
        HIP_TRY(hipEventCreate(&ev.e0));
        HIP_TRY(hipEventCreate(&ev.e1));
        HIP_TRY(hipEventRecord(ev.e0, c->stream));
    }
    const dim3 grid((unsigned)((ch->wp + UTM_GROUP_TILE_WORDS - 1) / UTM_GROUP_TILE_WORDS));  // one tile per workgroup, no cap
    const auto nt_of = [&](u64 columns) { return c->tune.nt_loads >= 0 ? c->tune.nt_loads != 0 : columns * ch->wp * 8 > ((u64)c->tune.nt_min_mb << 20); };
    if (nt_of(sorted.size()))
        hipLaunchKernelGGL((k_group_unions<true>), grid, dim3(256), 0, c->stream, (const u64 *)ch->cols, ch->wp, (const unsigned *)d_sorted.p,
                           (const unsigned *)d_offs.p, G, d_masks.p, d_totals.p);
    else
        hipLaunchKernelGGL((k_group_unions<false>), grid, dim3(256), 0, c->stream, (const u64 *)ch->cols, ch->wp, (const unsigned *)d_sorted.p,
                           (const unsigned *)d_offs.p, G, d_masks.p, d_totals.p);
    HIP_TRY(hipGetLastError());
    if (n) {
        // bin_mode 0 and 1: the head positions meet in LDS (there is room for at least UTM_GROUP_LDS_BINS / 128 = 64 of them)
        const unsigned R = bin_mode == 2 ? 0u : group_head(rows, (u64)n);
        const bool nt = nt_of((u64)n);
#define UTM_GROUP_LAUNCH(PRIV, NT)                                                                                                       \
    hipLaunchKernelGGL((k_group_curve<PRIV, NT>), grid, dim3(256), 0, c->stream, (const u64 *)ch->cols, ch->wp, (const unsigned *)d_order.p, \
                       (unsigned)n, (const u64 *)d_masks.p, G, R, d_bins.p)
        if (priv && nt) UTM_GROUP_LAUNCH(true, true);
        else if (priv) UTM_GROUP_LAUNCH(true, false);
        else if (nt) UTM_GROUP_LAUNCH(false, true);
        else UTM_GROUP_LAUNCH(false, false);
#undef UTM_GROUP_LAUNCH
        HIP_TRY(hipGetLastError());
    }
    if (pass_ms) HIP_TRY(hipEventRecord(ev.e1, c->stream));
    // into memory of this call first: the outputs stay untouched if a pass fails
    std::vector<i64> h_totals((size_t)2 * G), h_bins(cells);
    if (n) HIP_TRY(hipMemcpyAsync(h_bins.data(), d_bins.p, cells * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(copy_sync(c, h_totals.data(), d_totals.p, (size_t)2 * G * 8, hipMemcpyDeviceToHost));
    if (pass_ms) {
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, ev.e0, ev.e1));
        *pass_ms = ms;
    }
    std::copy(h_totals.begin(), h_totals.begin() + G, total_out);
    if (ptotal_out) std::copy(h_totals.begin() + G, h_totals.end(), ptotal_out);
    if (n) std::copy(h_bins.begin(), h_bins.begin() + (size_t)G * (size_t)n, new_out);
    if (n && priv) std::copy(h_bins.begin() + (size_t)G * (size_t)n, h_bins.end(), priv_out);
    return UTM_OK;
}

// The kernels' arithmetic built for the CPU, word by word: one chunk's columns (cols[s * wp + w], n_var <= 64 * wp
// variants, n_samp columns, padding bits zero), a group id per column and a list of n column indices; the outputs as
// utm_group_curve.  Needs no GPU.
extern "C" int utm_group_curve_host(const uint64_t *cols, uint64_t wp, uint64_t n_var, uint32_t n_samp, const int32_t *group_of, int32_t n_groups,
                                    const uint32_t *order, uint64_t n, int64_t *new_out, int64_t *priv_out, int64_t *total_out,
                                    int64_t *ptotal_out)
{
    if (!group_of || !total_out || (n && (!order || !new_out)) || (n_samp && !cols)) return fail(UTM_EINVAL, "NULL argument");
    if (n_var > wp * 64 || n > n_samp) return fail(UTM_EINVAL, "%llu variants in %llu words, %llu listed among %u samples", (unsigned long long)n_var,
                                                   (unsigned long long)wp, (unsigned long long)n, n_samp);
    std::vector<unsigned> sorted, offs, list;
    TRY(group_sort(group_of, n_samp, n_groups, &sorted, &offs));
    TRY(pair_list(order, n, n_samp, "order", &list));
    const u64 G = (u64)n_groups, words = (n_var + 63) / 64;
    std::vector<i64> fresh((size_t)(G * n), 0), priv((size_t)(priv_out ? G * n : 0), 0), total((size_t)G, 0), ptotal((size_t)G, 0);
    const u64 *q = (const u64 *)cols;
    u64 mask[UTM_GROUPS_MAX];
    for (u64 w = 0; w < words; ++w) {
        // k_group_unions: the groups' union words, closed into the two-plane counter one after the other
        u64 once = 0, twice = 0;
        for (u64 g = 0; g < G; ++g) {
            u64 u = 0;
            for (unsigned i = offs[(size_t)g]; i < offs[(size_t)g + 1]; ++i) u |= q[(u64)sorted[i] * wp + w];
            mask[g] = u;
            group_close(u, once, twice);
        }
        for (u64 g = 0; g < G; ++g) {
            total[(size_t)g] += __builtin_popcountll(mask[g]);
            ptotal[(size_t)g] += __builtin_popcountll(group_private(mask[g], twice));
        }
        // k_group_curve: the walk over the order; the masks are looked at only where a position captures something
        u64 cov = 0;
        for (u64 i = 0; i < n; ++i) {
            const u64 newly = group_newly(q[(u64)list[(size_t)i] * wp + w], cov);
            if (!newly) continue;
            for (u64 g = 0; g < G; ++g) {
                fresh[(size_t)(g * n + i)] += group_hits(newly, mask[g]);
                if (priv_out) priv[(size_t)(g * n + i)] += group_hits(group_private(newly, twice), mask[g]);
            }
        }
    }
    std::copy(total.begin(), total.end(), total_out);
    if (ptotal_out) std::copy(ptotal.begin(), ptotal.end(), ptotal_out);
    if (n) std::copy(fresh.begin(), fresh.end(), new_out);
    if (n && priv_out) std::copy(priv.begin(), priv.end(), priv_out);
    return UTM_OK;
}
