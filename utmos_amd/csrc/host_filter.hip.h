// Variant filters: utm_filter_variants (k_filter_prefix + k_filter_compact over one chunk) and the CPU build of its word
// arithmetic.  Part of the one translation unit utmos_hip.hip (included there, in order); not a stand-alone header.
#pragma once

// keep[] of a chunk with the bits at or above n_var cleared, and its set bits.
static u64 filter_clean_keep(const uint64_t *keep, u64 n_var, std::vector<u64> &clean)
{
    const u64 words = (n_var + 63) / 64;
    clean.assign(keep, keep + words);
    if (n_var & 63) clean[words - 1] &= (1ull << (n_var & 63)) - 1;
    u64 kept = 0;
    for (u64 w : clean) kept += (u64)__builtin_popcountll(w);
    return kept;
}

template <typename T>
static void filter_gather(std::vector<T> &values, const std::vector<u64> &keep)
{
    if (values.empty()) return;
    size_t n = 0;
    for (size_t v = 0; v < values.size(); ++v)
        if (keep[v >> 6] >> (v & 63) & 1) values[n++] = values[v];
    values.resize(n);
}

// Replaces, on the reference's side, filtering the VCF (bcftools view) before `utmos convert` and converting again: the
// reference has no way to restrict a loaded matrix to some of its variants.
extern "C" int utm_filter_variants(utm_ctx *c, int32_t chunk, const uint64_t *keep, uint64_t *n_kept, double *pass_ms)
{
    CTX(c);
    Chunk *ch;
    TRY(chunk_of(c, chunk, &ch));
    if (!keep) return fail(UTM_EINVAL, "keep is NULL");
    if (c->exported || c->p2p || c->comm)
        return fail(UTM_ESTATE, "the columns are exported to other shards, which have mapped their bases: filter the variants before "
                                "utm_p2p_export / utm_comm_init");
    std::vector<u64> clean;
    const u64 kept = filter_clean_keep(keep, ch->n_var, clean);
    if (pass_ms) *pass_ms = 0.0;
    if (n_kept) *n_kept = kept;
    if (kept == ch->n_var) {  // nothing to drop: the columns stay as they are, bit for bit
        c->prepared = false;  // (a restart, whatever the mask: the same state after every successful call)
        return UTM_OK;
    }

    // Out of place: the new column block (a chunk without variants keeps one zero KiB per column, so that every launch
    // shaped by wp still has a grid) and the new covered mask exist before anything of the old chunk is touched.
    const u64 w_in = ch->w, w_out = (kept + 63) / 64, wp_out = std::max<u64>(round_up(w_out, UTM_STEP_WORDS), UTM_STEP_WORDS);
    const size_t bytes = (size_t)c->n_local * wp_out * 8 + UTM_COLS_SLACK_BYTES;
    Scratch<u64> d_cols, d_covered, d_keep, d_prefix;
    if (d_cols.alloc(bytes / 8) != hipSuccess || d_covered.alloc(wp_out) != hipSuccess || d_keep.alloc(w_in) != hipSuccess ||
        d_prefix.alloc(w_in + 1) != hipSuccess) {
        (void)hipGetLastError();
        return fail(UTM_ENOMEM, "no room for the compacted chunk next to the matrix (%zu bytes): the chunk is unchanged", bytes);
    }
    HIP_TRY(hipMemsetAsync(d_cols.p, 0, bytes, c->stream));
    HIP_TRY(hipMemsetAsync(d_covered.p, 0, wp_out * 8, c->stream));
    HIP_TRY(hipMemcpyAsync(d_keep.p, clean.data(), w_in * 8, hipMemcpyHostToDevice, c->stream));
    struct Events {
        hipEvent_t e0 = nullptr, e1 = nullptr;
        ~Events() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
    } ev;
    if (pass_ms) {
        HIP_TRY(hipEventCreate(&ev.e0));
        HIP_TRY(hipEventCreate(&ev.e1));
        HIP_TRY(hipEventRecord(ev.e0, c->stream));
    }
    if (kept) {
        hipLaunchKernelGGL(k_filter_prefix, dim3(1), dim3(UTM_FILTER_SCAN_THREADS), 0, c->stream, (const u64 *)d_keep.p, w_in, d_prefix.p);
        TRY(launch_filter_compact(c, ch->cols, ch->wp, w_in, d_keep.p, d_prefix.p, d_cols.p, wp_out));  // (host_compact.hip.h)
    }
    if (pass_ms) HIP_TRY(hipEventRecord(ev.e1, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (pass_ms) {
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, ev.e0, ev.e1));
        *pass_ms = ms;
    }

    // The chunk becomes what utm_add_chunk + an upload of the kept rows would have made: everything derived from the old
    // columns goes (the next utm_reset builds what the run needs again, at the new size), the AF values are cut by the
    // same mask on the host, where they live -- the device tables are rebuilt from them at the reset anyway, and their
    // fixed-point unit follows the values that are left.
    (void)hipFree(ch->cols);
    (void)hipFree(ch->covered);
    ch->cols = d_cols.p;
    ch->covered = d_covered.p;
    d_cols.p = d_covered.p = nullptr;
    (void)hipFree(ch->covered_alt); ch->covered_alt = nullptr;
    (void)hipFree(ch->mask); ch->mask = nullptr;
    (void)hipFree(ch->list_idx); ch->list_idx = nullptr;
    (void)hipFree(ch->list_val); ch->list_val = nullptr;
    (void)hipFree(ch->rows_t); ch->rows_t = nullptr;
    (void)hipFree(ch->planes); ch->planes = nullptr;
    ch->rows_t_valid = false;
    filter_gather(ch->h_af32, clean);
    filter_gather(ch->h_af64, clean);
    c->n_var_total -= ch->n_var - kept;
    ch->n_var = kept;
    ch->w = w_out;
    ch->wp = wp_out;
    c->col_words = 0;
    for (auto &o : c->chunks) {
        o.off = c->col_words;
        c->col_words += o.wp;
    }
    c->dirty_tables = true;
    c->varcount_valid = false;
    c->prepared = false;
    return UTM_OK;
}

// The kernels' word arithmetic built for the CPU: every kept bit of cols[c * wp + w] lands at bit prefix + rank of
// out[c * wp_out + ...]; out is written whole, padding zero.  Needs no GPU.  (What it replaces: as utm_filter_variants.)
extern "C" int utm_filter_columns_host(const uint64_t *cols, uint64_t wp, uint64_t n_var, uint32_t n_cols, const uint64_t *keep,
                                       uint64_t *out, uint64_t wp_out, uint64_t *n_kept)
{
    if (!keep || (n_cols && (!cols || (!out && wp_out)))) return fail(UTM_EINVAL, "NULL argument");
    if (n_var > wp * 64) return fail(UTM_EINVAL, "%llu variants in %llu words", (unsigned long long)n_var, (unsigned long long)wp);
    std::vector<u64> clean;
    const u64 kept = filter_clean_keep(keep, n_var, clean);
    if (kept > wp_out * 64) return fail(UTM_EINVAL, "%llu kept variants in %llu words", (unsigned long long)kept, (unsigned long long)wp_out);
    if (n_kept) *n_kept = kept;
    const u64 words = clean.size();
    std::vector<u64> prefix(words + 1, 0);
    for (u64 w = 0; w < words; ++w) prefix[w + 1] = prefix[w] + (u64)__builtin_popcountll(clean[w]);
    std::fill(out, out + (size_t)n_cols * wp_out, (uint64_t)0);
    for (u64 w = 0; w < words; ++w) {
        if (!clean[w]) continue;
        FilterMasks f;
        filter_masks(clean[w], f);
        for (uint32_t c = 0; c < n_cols; ++c) {
            const u64 piece = filter_compress(cols[(u64)c * wp + w], f);
            if (!piece) continue;
            u64 lo, hi;
            filter_piece(piece, prefix[w], lo, hi);
            uint64_t *dst = out + (u64)c * wp_out + (prefix[w] >> 6);
            dst[0] |= lo;
            if (hi) dst[1] |= hi;
        }
    }
    return UTM_OK;
}
