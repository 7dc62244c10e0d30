// Pair counts: utm_pair_counts (k_swap_masks for a `given` list + k_pair_counts per chunk, the upper blocks mirrored on
// the host) and the CPU build of the same arithmetic.
// Part of the one translation unit utmos_hip.hip (included there, in order); not a stand-alone header.
#pragma once

// The kernel writes the blocks bj >= bi only (a diagonal block in full): the rest is their mirror image.
static void pair_mirror(i64 *x, u64 n)
{
    for (u64 i = 0; i < n; ++i)
        for (u64 j = (i / UTM_PAIR_B + 1) * UTM_PAIR_B; j < n; ++j) x[j * n + i] = x[i * n + j];
}

// A list of `count` sample indices below `limit`, each at most once -> unsigned; `what` names it in the message.
template <typename T>
static int pair_list(const T *list, u64 count, u64 limit, const char *what, std::vector<unsigned> *out)
{
    std::vector<unsigned char> listed((size_t)limit, 0);
    out->resize((size_t)count);
    for (u64 i = 0; i < count; ++i) {
        const i64 g = (i64)list[i];
        if (g < 0 || g >= (i64)limit)
            return fail(UTM_EINVAL, "%s entry %llu: sample %lld not in [0,%llu)", what, (unsigned long long)i, (long long)g, (unsigned long long)limit);
        if (listed[(size_t)g]) return fail(UTM_EINVAL, "%s entry %llu: sample %lld is listed twice", what, (unsigned long long)i, (long long)g);
        listed[(size_t)g] = 1;
        (*out)[(size_t)i] = (unsigned)g;
    }
    return UTM_OK;
}

extern "C" int utm_pair_counts(utm_ctx *c, const int64_t *global_idx, int64_t n, const int64_t *given, int64_t n_given, uint32_t tile_groups,
                               int64_t *out, double *pass_ms)
{
    CTX(c);
    if (n < 0 || n_given < 0 || (n > 0 && (!global_idx || !out)) || (n_given > 0 && !given)) return fail(UTM_EINVAL, "bad arguments");
    if (depth_sharded(c))
        return fail(UTM_ESTATE, "pair counts need the whole sample axis in one context without an exchange (this one holds samples "
                                "%u..%u of %u)", c->first, c->first + c->n_local, c->n_total);
    if (n > (i64)c->n_total || n_given > (i64)c->n_total)
        return fail(UTM_EINVAL, "lists of %lld and %lld, the matrix has %u samples", (long long)n, (long long)n_given, c->n_total);
    std::vector<unsigned> list, panel;
    TRY(pair_list(global_idx, (u64)n, c->n_total, "list", &list));
    TRY(pair_list(given, (u64)n_given, c->n_total, "given", &panel));
    if (pass_ms) *pass_ms = 0.0;
    if (n == 0) return UTM_OK;

    // Nothing of the context is read but the chunks' columns, and nothing of it is written: the lists, the masks, the
    // product and the events are this call's own.  The launches go on the context's stream, behind whatever wrote the columns.
    const u64 cells = (u64)n * (u64)n;
    u64 wp_max = 0;
    for (const Chunk &ch : c->chunks) wp_max = std::max(wp_max, ch.wp);
    Scratch<unsigned> d_list, d_panel;
    Scratch<u64> d_single, d_uncov, d_x;
    HIP_TRY(d_list.alloc((size_t)n));
    HIP_TRY(d_x.alloc((size_t)cells));
    HIP_TRY(hipMemcpyAsync(d_list.p, list.data(), (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    if (n_given) {
        HIP_TRY(d_panel.alloc((size_t)n_given));
        HIP_TRY(d_single.alloc((size_t)std::max<u64>(wp_max, 1)));
        HIP_TRY(d_uncov.alloc((size_t)std::max<u64>(wp_max, 1)));
        HIP_TRY(hipMemcpyAsync(d_panel.p, panel.data(), (size_t)n_given * 4, hipMemcpyHostToDevice, c->stream));
    }
    HIP_TRY(hipMemsetAsync(d_x.p, 0, (size_t)cells * 8, c->stream));
    struct Events {
        hipEvent_t e0 = nullptr, e1 = nullptr;
        ~Events() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
    } ev;
    if (pass_ms) {
        HIP_TRY(hipEventCreate(&ev.e0));
        HIP_TRY(hipEventCreate(&ev.e1));
        HIP_TRY(hipEventRecord(ev.e0, c->stream));
    }
    const u64 nb = ((u64)n + UTM_PAIR_B - 1) / UTM_PAIR_B, pairs = nb * (nb + 1) / 2;
    for (const Chunk &ch : c->chunks) {
        if (ch.n_var == 0) continue;
        const u64 tiles = (ch.wp + UTM_ORDER_TILE_WORDS - 1) / UTM_ORDER_TILE_WORDS;
        if (n_given)
            hipLaunchKernelGGL(k_swap_masks, dim3((unsigned)tiles), dim3(256), 0, c->stream, (const u64 *)ch.cols, ch.wp, ch.n_var,
                               (const unsigned *)d_panel.p, (unsigned)n_given, d_single.p, d_uncov.p);
        u64 groups = tile_groups ? (u64)tile_groups : std::max<u64>(1, UTM_SWAP_TARGET_WGS / pairs);
        groups = std::max(groups, (tiles + UTM_SWAP_MAX_TILES_PER_WG - 1) / UTM_SWAP_MAX_TILES_PER_WG);  // (an int32 accumulator per lane)
        groups = std::min<u64>(std::min(groups, tiles), 65535);                                        // (gridDim.y)
        // every listed column is read once per block of the list: past the caches' reach those reads stream
        const bool nt = c->tune.nt_loads >= 0 ? c->tune.nt_loads != 0 : (u64)n * ch.wp * 8 > ((u64)c->tune.nt_min_mb << 20);
        const dim3 grid((unsigned)pairs, (unsigned)groups);
        const u64 *mask = n_given ? (const u64 *)d_uncov.p : nullptr;
        if (nt)
            hipLaunchKernelGGL(k_pair_counts<true>, grid, dim3(256), 0, c->stream, (const u64 *)ch.cols, ch.wp, (const unsigned *)d_list.p, (unsigned)n, mask, d_x.p);
        else
            hipLaunchKernelGGL(k_pair_counts<false>, grid, dim3(256), 0, c->stream, (const u64 *)ch.cols, ch.wp, (const unsigned *)d_list.p, (unsigned)n, mask, d_x.p);
        HIP_TRY(hipGetLastError());
    }
    if (pass_ms) HIP_TRY(hipEventRecord(ev.e1, c->stream));
    // into memory of this call first: `out` stays untouched if a pass fails
    std::vector<i64> h((size_t)cells);
    HIP_TRY(copy_sync(c, h.data(), d_x.p, (size_t)cells * 8, hipMemcpyDeviceToHost));
    if (pass_ms) {
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, ev.e0, ev.e1));
        *pass_ms = ms;
    }
    pair_mirror(h.data(), (u64)n);
    std::copy(h.begin(), h.end(), out);
    return UTM_OK;
}

// The kernels' arithmetic built for the CPU, block pair by block pair as the grid walks them: one chunk's columns
// (cols[s * wp + w], n_var <= 64 * wp variants, n_samp columns, padding bits zero), a list of n column indices and a
// `given` list of n_given; out[n * n] as utm_pair_counts.  Needs no GPU.
extern "C" int utm_pair_counts_host(const uint64_t *cols, uint64_t wp, uint64_t n_var, uint32_t n_samp, const uint32_t *idx, uint64_t n,
                                    const uint32_t *given, uint64_t n_given, int64_t *out)
{
    if ((n && (!idx || !out || !cols)) || (n_given && (!given || !cols))) return fail(UTM_EINVAL, "NULL argument");
    if (n_var > wp * 64 || n > n_samp || n_given > n_samp)
        return fail(UTM_EINVAL, "%llu variants in %llu words, lists of %llu and %llu among %u samples", (unsigned long long)n_var,
                    (unsigned long long)wp, (unsigned long long)n, (unsigned long long)n_given, n_samp);
    std::vector<unsigned> list, panel;
    TRY(pair_list(idx, n, n_samp, "list", &list));
    TRY(pair_list(given, n_given, n_samp, "given", &panel));
    if (n == 0) return UTM_OK;
    const u64 *q = (const u64 *)cols;
    const u64 words = (n_var + 63) / 64;
    // the mask of k_swap_masks(panel = given); without a `given` list there is none
    std::vector<u64> uncov;
    if (n_given) {
        uncov.resize((size_t)words);
        for (u64 w = 0; w < words; ++w) {
            u64 once = 0, twice = 0;
            for (unsigned p : panel) swap_count(q[(u64)p * wp + w], once, twice);
            uncov[(size_t)w] = swap_uncovered(once, swap_valid(w, n_var));
        }
    }
    std::vector<i64> x((size_t)(n * n), 0);
    const unsigned nb = (unsigned)((n + UTM_PAIR_B - 1) / UTM_PAIR_B);
    std::vector<u64> staged(UTM_PAIR_B);
    for (unsigned p = 0; p < nb * (nb + 1) / 2; ++p) {
        unsigned bi, bj;
        pair_blocks(p, nb, bi, bj);
        const u64 i0 = (u64)bi * UTM_PAIR_B, j0 = (u64)bj * UTM_PAIR_B, i1 = std::min<u64>(n, i0 + UTM_PAIR_B), j1 = std::min<u64>(n, j0 + UTM_PAIR_B);
        for (u64 w = 0; w < words; ++w) {
            for (u64 j = j0; j < j1; ++j) staged[(size_t)(j - j0)] = n_given ? pair_stage(q[(u64)list[(size_t)j] * wp + w], uncov[(size_t)w]) : q[(u64)list[(size_t)j] * wp + w];
            for (u64 i = i0; i < i1; ++i) {
                const u64 row = bi == bj ? staged[(size_t)(i - i0)] : q[(u64)list[(size_t)i] * wp + w];
                if (!row) continue;
                for (u64 j = j0; j < j1; ++j) x[(size_t)(i * n + j)] += swap_pair(row, staged[(size_t)(j - j0)]);
            }
        }
    }
    pair_mirror(x.data(), n);
    std::copy(x.begin(), x.end(), out);
    return UTM_OK;
}
