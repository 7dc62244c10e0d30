// Class counts: utm_class_counts (one k_class_counts launch over one chunk) and the CPU build of the same arithmetic.
// Part of the one translation unit utmos_hip.hip (included there, in order); not a stand-alone header.
#pragma once

// Labels -1 .. n_classes-1 -> the packed labels of the kernel, `entries` >= n_var of them (the rest: counted nowhere).
static int class_labels(const int32_t *class_of, u64 n_var, i64 n_classes, u64 entries, std::vector<uint16_t> *out)
{
    out->assign((size_t)entries, (uint16_t)UTM_CLASS_NONE);
    for (u64 v = 0; v < n_var; ++v) {
        const int32_t c = class_of[v];
        if (c < -1 || c >= n_classes) return fail(UTM_EINVAL, "variant %llu: class %d not in -1..%lld", (unsigned long long)v, c, (long long)n_classes - 1);
        (*out)[(size_t)v] = class_pack(c);
    }
    return UTM_OK;
}

// The listed columns, or every column in index order for an empty list.
template <typename T>
static int class_list(const T *list, u64 count, u64 limit, std::vector<unsigned> *out)
{
    if (count) return pair_list(list, count, limit, "list", out);
    out->resize((size_t)limit);
    for (u64 i = 0; i < limit; ++i) (*out)[(size_t)i] = (unsigned)i;
    return UTM_OK;
}

extern "C" int utm_class_counts(utm_ctx *c, int32_t chunk, const int32_t *class_of, int32_t n_classes, const int64_t *global_idx, int64_t n,
                                uint32_t tile_groups, uint32_t mode, int64_t *table_out, double *pass_ms)
{
    CTX(c);
    if (!class_of || !table_out || n < 0 || (n > 0 && !global_idx)) return fail(UTM_EINVAL, "bad arguments");
    if (n_classes < 1 || n_classes > UTM_CLASSES_MAX) return fail(UTM_EINVAL, "%d classes not in 1..%d", n_classes, UTM_CLASSES_MAX);
    if (mode > 2) return fail(UTM_EINVAL, "mode %u not in 0..2", mode);
    Chunk *ch;
    TRY(chunk_of(c, chunk, &ch));
    if (depth_sharded(c))
        return fail(UTM_ESTATE, "class counts need the whole sample axis in one context without an exchange (this one holds samples "
                                "%u..%u of %u)", c->first, c->first + c->n_local, c->n_total);
    if (n > (i64)c->n_total) return fail(UTM_EINVAL, "a list of %lld, the matrix has %u samples", (long long)n, c->n_total);
    std::vector<unsigned> list;
    TRY(class_list(global_idx, (u64)n, c->n_total, &list));
    std::vector<uint16_t> labels;
    TRY(class_labels(class_of, ch->n_var, n_classes, ch->wp * 64, &labels));  // every word of the column has its 64 labels: no load can leave the buffer
    const u64 rows = list.size(), cells = rows * (u64)n_classes;
    const unsigned U = class_columns((unsigned)n_classes);
    const u64 blocks = (rows + U - 1) / U;
    if (blocks > 65535) return fail(UTM_EINVAL, "%llu listed samples in blocks of %u columns: gridDim.y holds 65,535 blocks", (unsigned long long)rows, U);
    if (pass_ms) *pass_ms = 0.0;
    if (ch->n_var == 0) {
        std::fill(table_out, table_out + cells, (int64_t)0);
        return UTM_OK;
    }

    // Nothing of the context is read but the chunk's columns, and nothing of it is written: the list, the labels, the table
    // and the events are this call's own.  The launch goes on the context's stream, behind whatever wrote the columns.
    Scratch<unsigned> d_list;
    Scratch<uint16_t> d_cls;
    Scratch<u64> d_table;
    HIP_TRY(d_list.alloc((size_t)rows));
    HIP_TRY(d_cls.alloc(labels.size()));
    HIP_TRY(d_table.alloc((size_t)cells));
    HIP_TRY(hipMemcpyAsync(d_list.p, list.data(), (size_t)rows * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(d_cls.p, labels.data(), labels.size() * 2, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(d_table.p, 0, (size_t)cells * 8, c->stream));
    struct Events {
        hipEvent_t e0 = nullptr, e1 = nullptr;
        ~Events() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
    } ev;
    if (pass_ms) {
        HIP_TRY(hipEventCreate(&ev.e0));
        HIP_TRY(hipEventCreate(&ev.e1));
        HIP_TRY(hipEventRecord(ev.e0, c->stream));
    }
    const u64 tiles = (ch->wp + UTM_CLASS_TILE_WORDS - 1) / UTM_CLASS_TILE_WORDS;
    u64 groups = tile_groups ? (u64)tile_groups : std::max<u64>(1, UTM_SWAP_TARGET_WGS / blocks);
    groups = std::max(groups, (tiles + UTM_SWAP_MAX_TILES_PER_WG - 1) / UTM_SWAP_MAX_TILES_PER_WG);  // (a 32-bit bin holds a workgroup's sum)
    groups = std::min(groups, tiles);
    // every listed column is read once: past the caches' reach those reads stream
    const bool nt = c->tune.nt_loads >= 0 ? c->tune.nt_loads != 0 : rows * ch->wp * 8 > ((u64)c->tune.nt_min_mb << 20);
    const dim3 grid((unsigned)groups, (unsigned)blocks);
    const size_t lds = (size_t)U * (size_t)n_classes * 4;
    // mode: 1 = the bit walk; 2 (popcounted head classes in front of the walk) is not built, so all three walk
    if (nt)
        hipLaunchKernelGGL(k_class_counts<true>, grid, dim3(256), lds, c->stream, (const u64 *)ch->cols, ch->wp, (const unsigned *)d_list.p, (unsigned)rows,
                           (const uint16_t *)d_cls.p, (unsigned)n_classes, d_table.p);
    else
        hipLaunchKernelGGL(k_class_counts<false>, grid, dim3(256), lds, c->stream, (const u64 *)ch->cols, ch->wp, (const unsigned *)d_list.p, (unsigned)rows,
                           (const uint16_t *)d_cls.p, (unsigned)n_classes, d_table.p);
    HIP_TRY(hipGetLastError());
    if (pass_ms) HIP_TRY(hipEventRecord(ev.e1, c->stream));
    // into memory of this call first: table_out stays untouched if the pass fails
    std::vector<i64> h((size_t)cells);
    HIP_TRY(copy_sync(c, h.data(), d_table.p, (size_t)cells * 8, hipMemcpyDeviceToHost));
    if (pass_ms) {
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, ev.e0, ev.e1));
        *pass_ms = ms;
    }
    std::copy(h.begin(), h.end(), table_out);
    return UTM_OK;
}

// The kernel's arithmetic built for the CPU, word by word: one chunk's columns (cols[s * wp + w], n_var <= 64 * wp
// variants, n_samp columns, padding bits zero), class_of[n_var], a list of n column indices (n == 0: every column, in
// index order); table_out[rows * n_classes] as utm_class_counts.  Needs no GPU.
extern "C" int utm_class_counts_host(const uint64_t *cols, uint64_t wp, uint64_t n_var, uint32_t n_samp, const int32_t *class_of, int32_t n_classes,
                                     const uint32_t *idx, uint64_t n, int64_t *table_out)
{
    if (!class_of || !table_out || (n && !idx) || (n_samp && n_var && !cols)) return fail(UTM_EINVAL, "NULL argument");
    if (n_classes < 1 || n_classes > UTM_CLASSES_MAX) return fail(UTM_EINVAL, "%d classes not in 1..%d", n_classes, UTM_CLASSES_MAX);
    if (n_var > wp * 64 || n > n_samp)
        return fail(UTM_EINVAL, "%llu variants in %llu words, a list of %llu among %u samples", (unsigned long long)n_var, (unsigned long long)wp,
                    (unsigned long long)n, n_samp);
    std::vector<unsigned> list;
    TRY(class_list(idx, n, n_samp, &list));
    const u64 words = (n_var + 63) / 64;
    std::vector<uint16_t> labels;
    TRY(class_labels(class_of, n_var, n_classes, words * 64, &labels));
    std::vector<i64> table(list.size() * (size_t)n_classes, 0);
    for (size_t j = 0; j < list.size(); ++j) {
        i64 *bins = table.data() + j * (size_t)n_classes;
        auto add = [bins](unsigned c) { ++bins[c]; };
        const u64 *col = (const u64 *)cols + (u64)list[j] * wp;
        for (u64 w = 0; w < words; ++w) class_word(col[w], labels.data() + w * 64, add);
    }
    std::copy(table.begin(), table.end(), table_out);
    return UTM_OK;
}
