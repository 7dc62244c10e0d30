// Carrier counts: utm_carrier_counts (k_swap_masks for a `given` list + one k_carrier_counts launch over one chunk) and
// the CPU build of the same arithmetic.
// Part of the one translation unit utmos_hip.hip (included there, in order); not a stand-alone header.
#pragma once

// The plane-count instantiation that holds counts up to n: 4, 8, 12, 16 or 20.
static int spectrum_planes_of(u64 n)
{
    int p = UTM_SPEC_LOW;
    while (n >> p) p += 4;
    return p;
}

template <int P>
static void launch_carrier_counts(utm_ctx *c, const Chunk &ch, bool nt, bool counts, const unsigned *d_list, unsigned n, const u64 *d_mask, int use_lds,
                                  u64 *d_hist, int32_t *d_count)
{
    const dim3 grid((unsigned)((ch.wp + UTM_SPEC_TILE_WORDS - 1) / UTM_SPEC_TILE_WORDS));  // one tile per workgroup, no cap
#define UTM_SPEC_LAUNCH(NT, COUNTS)                                                                                                   \
    hipLaunchKernelGGL((k_carrier_counts<P, NT, COUNTS>), grid, dim3(256), 0, c->stream, (const u64 *)ch.cols, ch.wp, ch.n_var, d_list, n, \
                       d_mask, use_lds, d_hist, d_count)
    if (nt && counts) UTM_SPEC_LAUNCH(true, true);
    else if (nt) UTM_SPEC_LAUNCH(true, false);
    else if (counts) UTM_SPEC_LAUNCH(false, true);
    else UTM_SPEC_LAUNCH(false, false);
#undef UTM_SPEC_LAUNCH
}

extern "C" int utm_carrier_counts(utm_ctx *c, int32_t chunk, const int64_t *global_idx, int64_t n, const int64_t *given, int64_t n_given,
                                  uint32_t hist_mode, int64_t *hist_out, int32_t *count_out, double *pass_ms)
{
    CTX(c);
    if (n < 0 || n_given < 0 || (n > 0 && !global_idx) || (n_given > 0 && !given) || (!hist_out && !count_out))
        return fail(UTM_EINVAL, "bad arguments");
    if (hist_mode > 2) return fail(UTM_EINVAL, "hist_mode %u not in 0..2", hist_mode);
    Chunk *ch;
    TRY(chunk_of(c, chunk, &ch));
    if (depth_sharded(c))
        return fail(UTM_ESTATE, "carrier counts need the whole sample axis in one context without an exchange (this one holds samples "
                                "%u..%u of %u)", c->first, c->first + c->n_local, c->n_total);
    if (n > (i64)UTM_SPEC_MAX_N) return fail(UTM_EINVAL, "%lld samples listed, the counter holds %u", (long long)n, UTM_SPEC_MAX_N);
    if (n > (i64)c->n_total || n_given > (i64)c->n_total)
        return fail(UTM_EINVAL, "lists of %lld and %lld, the matrix has %u samples", (long long)n, (long long)n_given, c->n_total);
    std::vector<unsigned> list, panel;
    TRY(pair_list(global_idx, (u64)n, c->n_total, "list", &list));
    TRY(pair_list(given, (u64)n_given, c->n_total, "given", &panel));
    const u64 bins = (u64)n + 1;
    if (hist_mode == 1 && bins > UTM_SPEC_LDS_BINS) return fail(UTM_EINVAL, "%llu bins, the LDS form holds %d", (unsigned long long)bins, UTM_SPEC_LDS_BINS);
    const int use_lds = hist_mode == 1 || (hist_mode == 0 && bins <= UTM_SPEC_LDS_BINS);
    if (pass_ms) *pass_ms = 0.0;
    if (ch->n_var == 0) {
        if (hist_out) std::fill(hist_out, hist_out + bins, (int64_t)0);
        return UTM_OK;
    }

    // Nothing of the context is read but the chunk's columns, and nothing of it is written: the lists, the mask, the bins,
    // the counts and the events are this call's own.  The launches go on the context's stream, behind whatever wrote the columns.
    Scratch<unsigned> d_list, d_panel;
    Scratch<u64> d_single, d_uncov, d_hist;
    Scratch<int32_t> d_count;
    const size_t entries = (size_t)ch->wp * 64;  // every word of the column has its 64 entries: no store can leave the buffer
    HIP_TRY(d_list.alloc((size_t)std::max<i64>(n, 1)));
    HIP_TRY(d_hist.alloc((size_t)bins));
    if (n) HIP_TRY(hipMemcpyAsync(d_list.p, list.data(), (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(d_hist.p, 0, (size_t)bins * 8, c->stream));
    if (n_given) {
        HIP_TRY(d_panel.alloc((size_t)n_given));
        HIP_TRY(d_single.alloc((size_t)ch->wp));
        HIP_TRY(d_uncov.alloc((size_t)ch->wp));
        HIP_TRY(hipMemcpyAsync(d_panel.p, panel.data(), (size_t)n_given * 4, hipMemcpyHostToDevice, c->stream));
    }
    if (count_out) {
        HIP_TRY(d_count.alloc(entries));
        HIP_TRY(hipMemsetAsync(d_count.p, n_given ? 0xFF : 0, entries * 4, c->stream));  // -1 under a mask, else 0: the kernel stores what differs
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
    if (n_given)
        hipLaunchKernelGGL(k_swap_masks, dim3((unsigned)((ch->wp + UTM_SWAP_TILE_WORDS - 1) / UTM_SWAP_TILE_WORDS)), dim3(256), 0, c->stream,
                           (const u64 *)ch->cols, ch->wp, ch->n_var, (const unsigned *)d_panel.p, (unsigned)n_given, d_single.p, d_uncov.p);
    const bool nt = c->tune.nt_loads >= 0 ? c->tune.nt_loads != 0 : (u64)n * ch->wp * 8 > ((u64)c->tune.nt_min_mb << 20);
    const u64 *d_mask = n_given ? (const u64 *)d_uncov.p : nullptr;
    switch (spectrum_planes_of((u64)n)) {
    case 4: launch_carrier_counts<4>(c, *ch, nt, count_out != nullptr, d_list.p, (unsigned)n, d_mask, use_lds, d_hist.p, d_count.p); break;
    case 8: launch_carrier_counts<8>(c, *ch, nt, count_out != nullptr, d_list.p, (unsigned)n, d_mask, use_lds, d_hist.p, d_count.p); break;
    case 12: launch_carrier_counts<12>(c, *ch, nt, count_out != nullptr, d_list.p, (unsigned)n, d_mask, use_lds, d_hist.p, d_count.p); break;
    case 16: launch_carrier_counts<16>(c, *ch, nt, count_out != nullptr, d_list.p, (unsigned)n, d_mask, use_lds, d_hist.p, d_count.p); break;
    default: launch_carrier_counts<20>(c, *ch, nt, count_out != nullptr, d_list.p, (unsigned)n, d_mask, use_lds, d_hist.p, d_count.p); break;
    }
    HIP_TRY(hipGetLastError());
    if (pass_ms) HIP_TRY(hipEventRecord(ev.e1, c->stream));
    // into memory of this call first: the outputs stay untouched if a pass fails
    std::vector<i64> h_hist((size_t)bins);
    std::vector<int32_t> h_count(count_out ? (size_t)ch->n_var : 0);
    if (count_out) HIP_TRY(hipMemcpyAsync(h_count.data(), d_count.p, (size_t)ch->n_var * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(copy_sync(c, h_hist.data(), d_hist.p, (size_t)bins * 8, hipMemcpyDeviceToHost));
    if (pass_ms) {
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, ev.e0, ev.e1));
        *pass_ms = ms;
    }
    if (hist_out) std::copy(h_hist.begin(), h_hist.end(), hist_out);
    if (count_out) std::copy(h_count.begin(), h_count.end(), count_out);
    return UTM_OK;
}

template <int P>
static void carrier_counts_host(const u64 *cols, u64 wp, u64 n_var, const std::vector<unsigned> &list, const std::vector<unsigned> &panel, i64 *hist,
                                int32_t *count)
{
    const u64 words = (n_var + 63) / 64, n = list.size();
    for (u64 w = 0; w < words; ++w) {
        u64 pl[P];
        for (int p = 0; p < P; ++p) pl[p] = 0;
        for (u64 i = 0; i < n; i += UTM_SPEC_B) {  // block by block, as the kernel's rounds
            u64 blk[UTM_SPEC_B];
            for (u64 u = 0; u < UTM_SPEC_B; ++u) blk[u] = i + u < n ? cols[(u64)list[(size_t)(i + u)] * wp + w] : 0ull;
            spectrum_block<P>(blk, pl);
        }
        // the mask of k_swap_masks(panel = given); without a `given` list the valid bits
        u64 once = 0, twice = 0;
        for (unsigned g : panel) swap_count(cols[(u64)g * wp + w], once, twice);
        const u64 valid = swap_valid(w, n_var), keep = panel.empty() ? valid : swap_uncovered(once, valid);
        unsigned low[UTM_SPEC_POP_BINS] = {0};
        u64 any;
        u64 rest = spectrum_low<P>(pl, keep, low, any);
        for (u64 b = 0; b < UTM_SPEC_POP_BINS && b <= n; ++b) hist[b] += low[b];
        for (; rest; rest &= rest - 1) ++hist[spectrum_count<P>(pl, __builtin_ctzll(rest))];
        if (!count) continue;
        // (count is filled as the device buffer is; it has only n_var entries, so padding is cut by `valid` in keep)
        for (u64 st = spectrum_store_bits(keep, any, !panel.empty()); st; st &= st - 1) {
            const int bit = __builtin_ctzll(st);
            count[w * 64 + (u64)bit] = (int32_t)spectrum_count<P>(pl, bit);
        }
    }
}

// The kernels' arithmetic built for the CPU, block of UTM_SPEC_B columns by block as the kernel walks them: one chunk's
// columns (cols[s * wp + w], n_var <= 64 * wp variants, n_samp columns, padding bits zero), a list of n column indices
// and a `given` list of n_given; hist_out[n + 1] and count_out[n_var] as utm_carrier_counts.  Needs no GPU.
extern "C" int utm_carrier_counts_host(const uint64_t *cols, uint64_t wp, uint64_t n_var, uint32_t n_samp, const uint32_t *idx, uint64_t n,
                                       const uint32_t *given, uint64_t n_given, int64_t *hist_out, int32_t *count_out)
{
    if ((n && !idx) || (n_given && !given) || (!hist_out && !count_out) || ((n || n_given) && !cols)) return fail(UTM_EINVAL, "NULL argument");
    if (n > UTM_SPEC_MAX_N) return fail(UTM_EINVAL, "%llu samples listed, the counter holds %u", (unsigned long long)n, UTM_SPEC_MAX_N);
    if (n_var > wp * 64 || n > n_samp || n_given > n_samp)
        return fail(UTM_EINVAL, "%llu variants in %llu words, lists of %llu and %llu among %u samples", (unsigned long long)n_var,
                    (unsigned long long)wp, (unsigned long long)n, (unsigned long long)n_given, n_samp);
    std::vector<unsigned> list, panel;
    TRY(pair_list(idx, n, n_samp, "list", &list));
    TRY(pair_list(given, n_given, n_samp, "given", &panel));
    std::vector<i64> hist((size_t)n + 1, 0);
    std::vector<int32_t> count(count_out ? (size_t)n_var : 0, n_given ? -1 : 0);
    const u64 *q = (const u64 *)cols;
    int32_t *cnt = count_out ? count.data() : nullptr;
    switch (spectrum_planes_of(n)) {
    case 4: carrier_counts_host<4>(q, wp, n_var, list, panel, hist.data(), cnt); break;
    case 8: carrier_counts_host<8>(q, wp, n_var, list, panel, hist.data(), cnt); break;
    case 12: carrier_counts_host<12>(q, wp, n_var, list, panel, hist.data(), cnt); break;
    case 16: carrier_counts_host<16>(q, wp, n_var, list, panel, hist.data(), cnt); break;
    default: carrier_counts_host<20>(q, wp, n_var, list, panel, hist.data(), cnt); break;
    }
    if (hist_out) std::copy(hist.begin(), hist.end(), hist_out);
    if (count_out) std::copy(count.begin(), count.end(), count_out);
    return UTM_OK;
}
