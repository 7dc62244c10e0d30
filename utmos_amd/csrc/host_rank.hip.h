// Capture ranks: utm_capture_rank (one k_capture_rank launch over one chunk) and the CPU build of its walk.
// Part of the one translation unit utmos_hip.hip (included there, in order); not a stand-alone header.
#pragma once

template <int P>
static void launch_capture_rank(utm_ctx *c, const Chunk &ch, bool nt, const unsigned *d_order, unsigned n, unsigned m, int32_t *d_rank)
{
    const dim3 grid((unsigned)((ch.wp + UTM_RANK_TILE_WORDS - 1) / UTM_RANK_TILE_WORDS));  // one tile per workgroup, no cap
    if (nt)
        hipLaunchKernelGGL((k_capture_rank<P, true>), grid, dim3(256), 0, c->stream, (const u64 *)ch.cols, ch.wp, d_order, n, m, d_rank);
    else
        hipLaunchKernelGGL((k_capture_rank<P, false>), grid, dim3(256), 0, c->stream, (const u64 *)ch.cols, ch.wp, d_order, n, m, d_rank);
}

extern "C" int utm_capture_rank(utm_ctx *c, int32_t chunk, const int64_t *global_idx, int64_t n, int32_t m, int32_t *rank_out,
                                double *pass_ms)
{
    CTX(c);
    if (!rank_out || n < 0 || (n > 0 && !global_idx)) return fail(UTM_EINVAL, "bad arguments");
    if (m < 1 || m > UTM_DEPTH_MAX) return fail(UTM_EINVAL, "depth %d not in 1..%d", m, UTM_DEPTH_MAX);
    Chunk *ch;
    TRY(chunk_of(c, chunk, &ch));
    if (depth_sharded(c))
        return fail(UTM_ESTATE, "capture ranks need the whole sample axis in one context without an exchange (this one holds samples "
                                "%u..%u of %u)", c->first, c->first + c->n_local, c->n_total);
    if (n > (i64)c->n_total || n > (i64)INT32_MAX) return fail(UTM_EINVAL, "%lld samples listed, the matrix has %u", (long long)n, c->n_total);
    std::vector<unsigned> order((size_t)n);
    {
        std::vector<unsigned char> listed(c->n_total, 0);
        for (i64 i = 0; i < n; ++i) {
            const i64 g = global_idx[i];
            if (g < 0 || g >= (i64)c->n_total) return fail(UTM_EINVAL, "entry %lld: sample %lld not in [0,%u)", (long long)i, (long long)g, c->n_total);
            if (listed[g]) return fail(UTM_EINVAL, "entry %lld: sample %lld is listed twice", (long long)i, (long long)g);
            listed[g] = 1;
            order[(size_t)i] = (unsigned)g;
        }
    }
    if (pass_ms) *pass_ms = 0.0;
    if (n == 0 || ch->n_var == 0) {
        std::fill(rank_out, rank_out + ch->n_var, (int32_t)-1);
        return UTM_OK;
    }

    // Nothing of the context is read but the chunk's columns, and nothing of it is written: the order, the ranks and the
    // two events are this call's own.  The launch goes on the context's stream, behind whatever wrote the columns.
    Scratch<unsigned> d_order;
    Scratch<int32_t> d_rank;
    const size_t entries = (size_t)ch->wp * 64;  // every word of the column has its 64 entries: no store can leave the buffer
    HIP_TRY(d_order.alloc((size_t)n));
    HIP_TRY(d_rank.alloc(entries));
    HIP_TRY(hipMemcpyAsync(d_order.p, order.data(), (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(d_rank.p, 0xFF, entries * 4, c->stream));
    struct Events {
        hipEvent_t e0 = nullptr, e1 = nullptr;
        ~Events() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
    } ev;
    if (pass_ms) {
        HIP_TRY(hipEventCreate(&ev.e0));
        HIP_TRY(hipEventCreate(&ev.e1));
        HIP_TRY(hipEventRecord(ev.e0, c->stream));
    }
    const bool nt = c->tune.nt_loads >= 0 ? c->tune.nt_loads != 0 : (u64)n * ch->wp * 8 > ((u64)c->tune.nt_min_mb << 20);
    switch (depth_planes_of(m)) {
    case 1: launch_capture_rank<1>(c, *ch, nt, d_order.p, (unsigned)n, (unsigned)m, d_rank.p); break;
    case 2: launch_capture_rank<2>(c, *ch, nt, d_order.p, (unsigned)n, (unsigned)m, d_rank.p); break;
    case 3: launch_capture_rank<3>(c, *ch, nt, d_order.p, (unsigned)n, (unsigned)m, d_rank.p); break;
    case 4: launch_capture_rank<4>(c, *ch, nt, d_order.p, (unsigned)n, (unsigned)m, d_rank.p); break;
    case 5: launch_capture_rank<5>(c, *ch, nt, d_order.p, (unsigned)n, (unsigned)m, d_rank.p); break;
    case 6: launch_capture_rank<6>(c, *ch, nt, d_order.p, (unsigned)n, (unsigned)m, d_rank.p); break;
    case 7: launch_capture_rank<7>(c, *ch, nt, d_order.p, (unsigned)n, (unsigned)m, d_rank.p); break;
    default: launch_capture_rank<8>(c, *ch, nt, d_order.p, (unsigned)n, (unsigned)m, d_rank.p); break;
    }
    HIP_TRY(hipGetLastError());
    if (pass_ms) HIP_TRY(hipEventRecord(ev.e1, c->stream));
    // into memory of this call first: rank_out stays untouched if the pass fails
    std::vector<int32_t> h((size_t)ch->n_var);
    HIP_TRY(copy_sync(c, h.data(), d_rank.p, (size_t)ch->n_var * 4, hipMemcpyDeviceToHost));
    if (pass_ms) {
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, ev.e0, ev.e1));
        *pass_ms = ms;
    }
    std::copy(h.begin(), h.end(), rank_out);
    return UTM_OK;
}

template <int P>
static void capture_rank_host(const u64 *cols, u64 wp, u64 n_var, const uint32_t *order, u64 n, unsigned m, int32_t *rank_out)
{
    const u64 words = (n_var + 63) / 64;
    for (u64 w = 0; w < words; ++w) {
        // (the kernel relies on zero padding; rank_out has only n_var entries, so the last word's padding is cut here)
        const u64 valid = (w + 1) * 64 <= n_var ? ~0ull : (1ull << (n_var & 63)) - 1;
        u64 cov = 0, pl[P];
        for (int p = 0; p < P; ++p) pl[p] = 0;
        for (u64 i = 0; i < n; ++i) rank_store(rank_out + w * 64, rank_word<P>(cols[(u64)order[i] * wp + w], cov, pl, m) & valid, (int32_t)i);
    }
}

// The kernel's walk built for the CPU: one chunk's columns (cols[s * wp + w]), a list of n column indices and a depth m;
// rank_out[v], v < n_var = the position at which m listed columns carry v, or -1.  Needs no GPU.
extern "C" int utm_capture_rank_host(const uint64_t *cols, uint64_t wp, uint64_t n_var, const uint32_t *order, uint64_t n, int32_t m,
                                     int32_t *rank_out)
{
    if (!rank_out || (n && (!order || !cols))) return fail(UTM_EINVAL, "NULL argument");
    if (m < 1 || m > UTM_DEPTH_MAX) return fail(UTM_EINVAL, "depth %d not in 1..%d", m, UTM_DEPTH_MAX);
    if (n_var > wp * 64 || n > (u64)INT32_MAX) return fail(UTM_EINVAL, "%llu variants in %llu words, %llu listed", (unsigned long long)n_var, (unsigned long long)wp, (unsigned long long)n);
    std::fill(rank_out, rank_out + n_var, (int32_t)-1);
    const u64 *q = (const u64 *)cols;
    switch (depth_planes_of(m)) {
    case 1: capture_rank_host<1>(q, wp, n_var, order, n, (unsigned)m, rank_out); break;
    case 2: capture_rank_host<2>(q, wp, n_var, order, n, (unsigned)m, rank_out); break;
    case 3: capture_rank_host<3>(q, wp, n_var, order, n, (unsigned)m, rank_out); break;
    case 4: capture_rank_host<4>(q, wp, n_var, order, n, (unsigned)m, rank_out); break;
    case 5: capture_rank_host<5>(q, wp, n_var, order, n, (unsigned)m, rank_out); break;
    case 6: capture_rank_host<6>(q, wp, n_var, order, n, (unsigned)m, rank_out); break;
    case 7: capture_rank_host<7>(q, wp, n_var, order, n, (unsigned)m, rank_out); break;
    default: capture_rank_host<8>(q, wp, n_var, order, n, (unsigned)m, rank_out); break;
    }
    return UTM_OK;
}
