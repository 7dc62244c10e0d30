// Coverage depth: utm_set_depth, the launches of k_depth_apply, utm_get_support / utm_get_at_depth and the CPU build
// of the word arithmetic.
// Part of the one translation unit utmos_hip.hip (included there, in order); not a stand-alone header.
#pragma once

static int flush_pending(utm_ctx *c);
static int ensure_prepared(utm_ctx *c);

// A context that holds a shard of the samples, or has any exchange set up: depth is not built for those.
static bool depth_sharded(const utm_ctx *c)
{
    return c->n_local != c->n_total || c->n_ranks != 1 || c->comm || c->p2p || mailbox_exchange(c);
}

static int depth_planes_of(int m)
{
    int p = 0;
    while (m >> p) ++p;
    return p;
}

static void depth_free(utm_ctx *c)
{
    for (auto &ch : c->chunks) {
        (void)hipFree(ch.planes);
        ch.planes = nullptr;
    }
    (void)hipFree(c->d_depth_acc);
    (void)hipFree(c->d_depth_sync);
    (void)hipFree(c->d_res_sat);
    c->d_depth_acc = nullptr;
    c->d_depth_sync = nullptr;
    c->d_res_sat = nullptr;
}

extern "C" int utm_set_depth(utm_ctx *c, int32_t m)
{
    CTX(c);
    if (m < 1 || m > UTM_DEPTH_MAX) return fail(UTM_EINVAL, "depth %d not in 1..%d", m, UTM_DEPTH_MAX);
    if (m > 1 && depth_sharded(c))
        return fail(UTM_ESTATE, "a coverage depth above 1 needs the whole sample axis in one context without an exchange (this one holds "
                                "samples %u..%u of %u)", c->first, c->first + c->n_local, c->n_total);
    if (m == c->depth) return UTM_OK;
    HIP_TRY(hipStreamSynchronize(c->stream));
    depth_free(c);  // (the plane count follows M; M = 1 keeps nothing)
    c->depth = m;
    c->depth_launches = 0;
    c->depth_ms = 0;
    c->ev_depth_used = 0;
    c->depth_planes = m > 1 ? depth_planes_of(m) : 0;
    // everything that rests on "covered only grows by the winner's column" is off while M > 1
    c->decr_enabled = c->decr_requested && m == 1;
    c->prepared = false;
    return UTM_OK;
}

// utm_reset, M > 1: planes, sums and the per-row record exist and are zero.
static int depth_prepare(utm_ctx *c)
{
    if (c->depth <= 1) return UTM_OK;
    if (depth_sharded(c)) return fail(UTM_ESTATE, "a coverage depth above 1 cannot run on a shard or with an exchange set up");
    for (auto &ch : c->chunks) {
        if (!ch.planes) HIP_TRY(hipMalloc(&ch.planes, (size_t)c->depth_planes * ch.wp * 8));
        HIP_TRY(hipMemsetAsync(ch.planes, 0, (size_t)c->depth_planes * ch.wp * 8, c->stream));
    }
    if (!c->d_depth_acc) HIP_TRY(hipMalloc(&c->d_depth_acc, 16));
    if (!c->d_depth_sync) HIP_TRY(hipMalloc(&c->d_depth_sync, sizeof(DepthSync)));
    if (!c->d_res_sat) HIP_TRY(hipMalloc(&c->d_res_sat, ((size_t)c->n_total + 1) * 8));
    HIP_TRY(hipMemsetAsync(c->d_depth_acc, 0, 16, c->stream));
    HIP_TRY(hipMemsetAsync(c->d_depth_sync, 0, sizeof(DepthSync), c->stream));
    HIP_TRY(hipMemsetAsync(c->d_res_sat, 0, ((size_t)c->n_total + 1) * 8, c->stream));
    c->depth_launches = 0;
    c->depth_ms = 0;
    c->ev_depth_used = 0;
    if (getenv("UTM_VERBOSE"))
        fprintf(stderr, "libutmos_hip: depth %d (%d planes): every iteration is a full scoring pass plus k_depth_apply; the persistent loop%s, "
                        "AF delta passes and deferred scores are off\n", c->depth, c->depth_planes,
                c->decr_requested ? ", decremental scoring (requested)" : "");
    return UTM_OK;
}

// One chunk, one column: `col` = a column named by the host, or nullptr = the pending winner (a launch of the loop; the
// launch of the last chunk commits the row).  units / sat: where the launch adds its two sums.
static void launch_depth_apply(utm_ctx *c, const Chunk &ch, const u64 *col, u64 *units, u64 *sat, bool commit)
{
    hipEvent_t start = nullptr, stop = nullptr;
    if (c->flags & UTM_FLAG_PROFILE_EVENTS) {
        if (c->ev_depth_used + 2 > c->ev_depth.size()) {
            hipEvent_t a, b;
            (void)hipEventCreate(&a);
            (void)hipEventCreate(&b);
            c->ev_depth.push_back(a);
            c->ev_depth.push_back(b);
        }
        start = c->ev_depth[c->ev_depth_used];
        stop = c->ev_depth[c->ev_depth_used + 1];
        c->ev_depth_used += 2;
    }
    c->depth_launches += 1;
    const dim3 grid((unsigned)std::min<u64>(1024, (ch.wp / 2 + 255) / 256));
    DepthSync *sync = col ? nullptr : c->d_depth_sync;
#define UTM_LAUNCH_DEPTH(P)                                                                                                      \
    hipExtLaunchKernelGGL(k_depth_apply<P>, grid, dim3(256), 0, c->stream, start, stop, 0, ch.covered, ch.planes, (const u64 *)ch.cols, \
                          ch.wp, pending_of(c, ch, false), c->d_st, col, (unsigned)c->depth, units, sat, sync, c->d_res_sat, commit ? 1 : 0)
    switch (c->depth_planes) {
    case 2: UTM_LAUNCH_DEPTH(2); break;
    case 3: UTM_LAUNCH_DEPTH(3); break;
    case 4: UTM_LAUNCH_DEPTH(4); break;
    case 5: UTM_LAUNCH_DEPTH(5); break;
    case 6: UTM_LAUNCH_DEPTH(6); break;
    case 7: UTM_LAUNCH_DEPTH(7); break;
    default: UTM_LAUNCH_DEPTH(8); break;
    }
#undef UTM_LAUNCH_DEPTH
}

// The loop's launch after a pick: the winner goes into the planes of every chunk, nothing stays pending.
static int enqueue_depth_apply(utm_ctx *c)
{
    for (size_t k = 0; k < c->chunks.size(); ++k)
        launch_depth_apply(c, c->chunks[k], nullptr, c->d_depth_acc, c->d_depth_acc + 1, k + 1 == c->chunks.size());
    HIP_TRY(hipGetLastError());
    return UTM_OK;
}

static int collect_depth_times(utm_ctx *c)
{
    for (size_t i = 0; i + 1 < c->ev_depth_used; i += 2) {
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, c->ev_depth[i], c->ev_depth[i + 1]));
        c->depth_ms += ms;
    }
    c->ev_depth_used = 0;
    return UTM_OK;
}

extern "C" int utm_get_depth(utm_ctx *c, int32_t *m, int64_t *apply_launches, double *apply_ms)
{
    CTX(c);
    if (m) *m = c->depth;
    if (apply_launches) *apply_launches = c->depth_launches;
    if (apply_ms) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        TRY(collect_depth_times(c));
        *apply_ms = c->depth_ms;
    }
    return UTM_OK;
}

extern "C" int utm_get_at_depth(utm_ctx *c, int64_t first_row, int64_t n_rows, int64_t *out)
{
    CTX(c);
    if (c->depth <= 1) return fail(UTM_ESTATE, "the depth is 1: the rows' tot_captured is the number of saturated variants");
    if (first_row < 0 || n_rows < 0 || (n_rows > 0 && !out)) return fail(UTM_EINVAL, "bad arguments");
    TRY(ensure_prepared(c));
    if (first_row + n_rows > c->iter) return fail(UTM_EINVAL, "rows %lld..%lld of %lld", (long long)first_row, (long long)(first_row + n_rows), (long long)c->iter);
    if (n_rows) HIP_TRY(copy_sync(c, out, c->d_res_sat + first_row, (size_t)n_rows * 8, hipMemcpyDeviceToHost));
    return UTM_OK;
}

extern "C" int utm_get_support(utm_ctx *c, int32_t chunk, uint8_t *out)
{
    CTX(c);
    Chunk *ch;
    TRY(chunk_of(c, chunk, &ch));
    if (!out) return fail(UTM_EINVAL, "out is NULL");
    TRY(ensure_prepared(c));
    const int planes = c->depth > 1 ? c->depth_planes : 1;
    std::vector<u64> h((size_t)planes * ch->w);
    if (c->depth > 1) {
        for (int p = 0; p < planes; ++p)
            HIP_TRY(hipMemcpyAsync(h.data() + (size_t)p * ch->w, ch->planes + (u64)p * ch->wp, ch->w * 8, hipMemcpyDeviceToHost, c->stream));
    } else {  // M = 1: the support is the covered bit (pending winner applied, as utm_get_covered does)
        c->keep_valid = false;
        TRY(flush_pending(c));
        HIP_TRY(hipMemcpyAsync(h.data(), ch->covered, ch->w * 8, hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (u64 v = 0; v < ch->n_var; ++v) {
        unsigned s = 0;
        for (int p = 0; p < planes; ++p) s |= (unsigned)(h[(size_t)p * ch->w + (v >> 6)] >> (v & 63) & 1ull) << p;
        out[v] = (uint8_t)s;
    }
    return UTM_OK;
}

template <int P>
static void depth_apply_host(const u64 *col, u64 wp, u64 *covered, u64 *planes, unsigned m, u64 *units, u64 *newly)
{
    for (u64 w = 0; w < wp; ++w) {
        u64 pl[P];
        for (int p = 0; p < P; ++p) pl[p] = planes[(u64)p * wp + w];
        unsigned u = 0, n = 0;
        depth_word<P>(col[w], covered[w], pl, m, u, n);
        for (int p = 0; p < P; ++p) planes[(u64)p * wp + w] = pl[p];
        *units += u;
        *newly += n;
    }
}

// k_depth_apply's walk built for the CPU: one column of wp words into covered[wp] and planes[p * wp + w],
// p < bit_length(m), all updated in place; *units += the units gained, *newly_saturated += the variants that reached m.
// Needs no GPU.
extern "C" int utm_depth_apply_host(const uint64_t *col, uint64_t wp, uint64_t *covered, uint64_t *planes, int32_t m, uint64_t *units,
                                    uint64_t *newly_saturated)
{
    if (!col || !covered || !planes || !units || !newly_saturated) return fail(UTM_EINVAL, "NULL argument");
    if (m < 1 || m > UTM_DEPTH_MAX) return fail(UTM_EINVAL, "depth %d not in 1..%d", m, UTM_DEPTH_MAX);
    u64 *cov = reinterpret_cast<u64 *>(covered), *pl = reinterpret_cast<u64 *>(planes);
    u64 u = 0, n = 0;
    switch (depth_planes_of(m)) {
    case 1: depth_apply_host<1>((const u64 *)col, wp, cov, pl, (unsigned)m, &u, &n); break;
    case 2: depth_apply_host<2>((const u64 *)col, wp, cov, pl, (unsigned)m, &u, &n); break;
    case 3: depth_apply_host<3>((const u64 *)col, wp, cov, pl, (unsigned)m, &u, &n); break;
    case 4: depth_apply_host<4>((const u64 *)col, wp, cov, pl, (unsigned)m, &u, &n); break;
    case 5: depth_apply_host<5>((const u64 *)col, wp, cov, pl, (unsigned)m, &u, &n); break;
    case 6: depth_apply_host<6>((const u64 *)col, wp, cov, pl, (unsigned)m, &u, &n); break;
    case 7: depth_apply_host<7>((const u64 *)col, wp, cov, pl, (unsigned)m, &u, &n); break;
    default: depth_apply_host<8>((const u64 *)col, wp, cov, pl, (unsigned)m, &u, &n); break;
    }
    *units += u;
    *newly_saturated += n;
    return UTM_OK;
}
