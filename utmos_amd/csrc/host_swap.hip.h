// Swap gains: utm_swap_gains (k_swap_masks + k_swap_pairs per chunk, the gains put together on the host) and the CPU
// build of the same arithmetic.
// Part of the one translation unit utmos_hip.hip (included there, in order); not a stand-alone header.
#pragma once

// gain[i][t] = g_t + x[i][t] - u_i from the product x[(k + 1)][n + 1] (row k: g and the missed variants, column n: u).
static void swap_gains_from_product(const i64 *x, u64 k, u64 n, i64 n_var, int64_t *gain_out, int64_t *unique_out, int64_t *new_out,
                                    int64_t *base_out)
{
    const i64 *g = x + k * (n + 1);
    for (u64 i = 0; i < k; ++i) {
        const i64 *xi = x + i * (n + 1);
        for (u64 t = 0; t < n; ++t) gain_out[i * n + t] = g[t] + xi[t] - xi[n];
        if (unique_out) unique_out[i] = xi[n];
    }
    if (new_out) std::copy(g, g + n, new_out);
    if (base_out) *base_out = n_var - g[n];
}

#define UTM_SWAP_TARGET_WGS 8192  // workgroups of a k_swap_pairs launch, about: tile groups = this / (candidate x row blocks)

extern "C" int utm_swap_gains(utm_ctx *c, const int64_t *panel, int64_t k, int64_t *gain_out, int64_t *unique_out, int64_t *new_out,
                              int64_t *base_out, double *pass_ms)
{
    CTX(c);
    if (k < 0 || (k > 0 && (!panel || !gain_out))) return fail(UTM_EINVAL, "bad arguments");
    if (depth_sharded(c))
        return fail(UTM_ESTATE, "swap gains need the whole sample axis in one context without an exchange (this one holds samples "
                                "%u..%u of %u)", c->first, c->first + c->n_local, c->n_total);
    if (k > (i64)c->n_total) return fail(UTM_EINVAL, "a panel of %lld, the matrix has %u samples", (long long)k, c->n_total);
    std::vector<unsigned> members((size_t)k);
    {
        std::vector<unsigned char> listed(c->n_total, 0);
        for (i64 i = 0; i < k; ++i) {
            const i64 g = panel[i];
            if (g < 0 || g >= (i64)c->n_total) return fail(UTM_EINVAL, "entry %lld: sample %lld not in [0,%u)", (long long)i, (long long)g, c->n_total);
            if (listed[g]) return fail(UTM_EINVAL, "entry %lld: sample %lld is listed twice", (long long)i, (long long)g);
            listed[g] = 1;
            members[(size_t)i] = (unsigned)g;
        }
    }
    if (pass_ms) *pass_ms = 0.0;
    if (k == 0) {
        if (base_out) *base_out = 0;
        return UTM_OK;
    }

    // Nothing of the context is read but the chunks' columns, and nothing of it is written: the panel, the two masks, the
    // product and the events are this call's own.  The launches go on the context's stream, behind whatever wrote the columns.
    const u64 n = c->n_total, rows = (u64)k + 1, cells = rows * (n + 1);
    u64 wp_max = 0;
    for (const Chunk &ch : c->chunks) wp_max = std::max(wp_max, ch.wp);
    Scratch<unsigned> d_panel;
    Scratch<u64> d_single, d_uncov, d_x;
    HIP_TRY(d_panel.alloc((size_t)k));
    HIP_TRY(d_single.alloc((size_t)std::max<u64>(wp_max, 1)));
    HIP_TRY(d_uncov.alloc((size_t)std::max<u64>(wp_max, 1)));
    HIP_TRY(d_x.alloc((size_t)cells));
    HIP_TRY(hipMemcpyAsync(d_panel.p, members.data(), (size_t)k * 4, hipMemcpyHostToDevice, c->stream));
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
    const unsigned cand_blocks = (unsigned)((n + 1 + UTM_SWAP_T - 1) / UTM_SWAP_T), row_blocks = (unsigned)((rows + 63) / 64);
    i64 n_var = 0;
    for (const Chunk &ch : c->chunks) {
        n_var += (i64)ch.n_var;
        if (ch.n_var == 0) continue;
        const u64 tiles = (ch.wp + UTM_SWAP_TILE_WORDS - 1) / UTM_SWAP_TILE_WORDS;
        hipLaunchKernelGGL(k_swap_masks, dim3((unsigned)tiles), dim3(256), 0, c->stream, (const u64 *)ch.cols, ch.wp, ch.n_var, (const unsigned *)d_panel.p,
                           (unsigned)k, d_single.p, d_uncov.p);
        u64 groups = std::max<u64>(1, UTM_SWAP_TARGET_WGS / ((u64)cand_blocks * row_blocks));
        groups = std::max(groups, (tiles + UTM_SWAP_MAX_TILES_PER_WG - 1) / UTM_SWAP_MAX_TILES_PER_WG);  // (an int32 accumulator per lane)
        groups = std::min(groups, tiles);
        hipLaunchKernelGGL(k_swap_pairs, dim3((unsigned)groups, cand_blocks, row_blocks), dim3(256), 0, c->stream, (const u64 *)ch.cols, ch.wp, (unsigned)n,
                           (const unsigned *)d_panel.p, (unsigned)k, (const u64 *)d_single.p, (const u64 *)d_uncov.p, d_x.p);
        HIP_TRY(hipGetLastError());
    }
    if (pass_ms) HIP_TRY(hipEventRecord(ev.e1, c->stream));
    // into memory of this call first: the outputs stay untouched if a pass fails
    std::vector<i64> h((size_t)cells);
    HIP_TRY(copy_sync(c, h.data(), d_x.p, (size_t)cells * 8, hipMemcpyDeviceToHost));
    if (pass_ms) {
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, ev.e0, ev.e1));
        *pass_ms = ms;
    }
    swap_gains_from_product(h.data(), (u64)k, n, n_var, gain_out, unique_out, new_out, base_out);
    return UTM_OK;
}

// The two kernels' arithmetic built for the CPU: one chunk's columns (cols[s * wp + w], n_var <= 64 * wp variants, n_samp
// columns) and a panel of k column indices; the outputs of utm_swap_gains.  Needs no GPU.
extern "C" int utm_swap_gains_host(const uint64_t *cols, uint64_t wp, uint64_t n_var, uint32_t n_samp, const uint32_t *panel, uint64_t k,
                                   int64_t *gain_out, int64_t *unique_out, int64_t *new_out, int64_t *base_out)
{
    if (k && (!panel || !gain_out || !cols)) return fail(UTM_EINVAL, "NULL argument");
    if (n_var > wp * 64 || k > n_samp) return fail(UTM_EINVAL, "%llu variants in %llu words, a panel of %llu among %u samples", (unsigned long long)n_var,
                                                   (unsigned long long)wp, (unsigned long long)k, n_samp);
    {
        std::vector<unsigned char> listed(n_samp, 0);
        for (u64 i = 0; i < k; ++i) {
            if (panel[i] >= n_samp) return fail(UTM_EINVAL, "entry %llu: sample %u not in [0,%u)", (unsigned long long)i, panel[i], n_samp);
            if (listed[panel[i]]) return fail(UTM_EINVAL, "entry %llu: sample %u is listed twice", (unsigned long long)i, panel[i]);
            listed[panel[i]] = 1;
        }
    }
    if (k == 0) {
        if (base_out) *base_out = 0;
        return UTM_OK;
    }
    const u64 *q = (const u64 *)cols;
    const u64 n = n_samp, words = (n_var + 63) / 64;
    // stage 1: the two masks
    std::vector<u64> single(words), uncov(words);
    for (u64 w = 0; w < words; ++w) {
        u64 once = 0, twice = 0;
        for (u64 i = 0; i < k; ++i) swap_count(q[(u64)panel[i] * wp + w], once, twice);
        single[w] = swap_single(once, twice);
        uncov[w] = swap_uncovered(once, swap_valid(w, n_var));
    }
    // stage 2: the product, candidate n = all ones
    std::vector<i64> x((k + 1) * (n + 1), 0);
    for (u64 r = 0; r <= k; ++r) {
        i64 *xr = x.data() + r * (n + 1);
        for (u64 w = 0; w < words; ++w) {
            const u64 row = r < k ? q[(u64)panel[r] * wp + w] & single[w] : uncov[w];
            if (!row) continue;
            for (u64 t = 0; t < n; ++t) xr[t] += swap_pair(row, q[t * wp + w]);
            xr[n] += swap_pair(row, ~0ull);
        }
    }
    swap_gains_from_product(x.data(), k, n, (i64)n_var, gain_out, unique_out, new_out, base_out);
    return UTM_OK;
}
