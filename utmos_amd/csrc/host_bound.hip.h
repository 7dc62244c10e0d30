// Coverage bound: utm_coverage_bound (k_swap_masks + k_bound_init per chunk, then per iteration k_bound_sums per chunk,
// one k_bound_pick and k_bound_update per chunk, all enqueued at once) and the CPU build of the same arithmetic.
// Part of the one translation unit utmos_hip.hip (included there, in order); not a stand-alone header.
#pragma once

struct BoundArgs {
    i64 kk;            // min(k, n_cand)
    unsigned step0, period;
};

// The checks both entry points share (the lists are checked by their callers: their index types differ).
static int bound_args(i64 n_cand, i64 k, int32_t iters, uint32_t step0, uint32_t period, const int64_t *hist_out, BoundArgs *a)
{
    if (!hist_out) return fail(UTM_EINVAL, "hist_out is NULL");
    if (k < 1) return fail(UTM_EINVAL, "k = %lld: a panel has at least one sample", (long long)k);
    if (iters < 1 || iters > 65535) return fail(UTM_EINVAL, "%d iterations, not in 1..65535", iters);
    if (step0 > UTM_BOUND_Q) return fail(UTM_EINVAL, "step0 = %u above %u", step0, UTM_BOUND_Q);
    a->kk = std::min<i64>(k, n_cand);
    a->step0 = step0 ? step0 : UTM_BOUND_Q / 4;
    a->period = period ? period : (unsigned)std::max(1, iters / 14);
    return UTM_OK;
}

// bound = min(n_live, min_t floor(L_t / Q)), best_iter = the first t at that minimum.
static void bound_from_hist(const i64 *hist, int32_t iters, i64 n_live, int64_t *bound_out, int32_t *best_iter_out, int64_t *n_live_out)
{
    i64 best = hist[0] / (i64)UTM_BOUND_Q;
    int32_t at = 0;
    for (int32_t t = 1; t < iters; ++t)
        if (hist[t] / (i64)UTM_BOUND_Q < best) best = hist[t] / (i64)UTM_BOUND_Q, at = t;
    if (bound_out) *bound_out = std::min(best, n_live);
    if (best_iter_out) *best_iter_out = at;
    if (n_live_out) *n_live_out = n_live;
}

// HIP events around every launch of the three per-iteration kernels, on a context created with UTM_FLAG_PROFILE_EVENTS only
// (tools/bound_bench.py); utm_coverage_bound_times returns their sums.
struct BoundTimers {
    bool on = false;
    std::vector<hipEvent_t> ev;  // pairs
    std::vector<int> kind;       // 0 sums, 1 pick, 2 update
    ~BoundTimers() { for (auto e : ev) (void)hipEventDestroy(e); }
    void pair(int k, hipEvent_t *start, hipEvent_t *stop)
    {
        *start = *stop = nullptr;
        if (!on) return;
        hipEvent_t a = nullptr, b = nullptr;
        if (hipEventCreate(&a) != hipSuccess) return;
        if (hipEventCreate(&b) != hipSuccess) { (void)hipEventDestroy(a); return; }
        ev.push_back(a); ev.push_back(b); kind.push_back(k);
        *start = a; *stop = b;
    }
};

template <typename T>
static int bound_list(const T *list, i64 n, u64 n_samp, const char *what, std::vector<unsigned> *out)
{
    if (n < 0 || (n > 0 && !list)) return fail(UTM_EINVAL, "%s: a NULL list of %lld", what, (long long)n);
    if ((u64)n > n_samp) return fail(UTM_EINVAL, "%s: %lld entries, the matrix has %llu samples", what, (long long)n, (unsigned long long)n_samp);
    std::vector<unsigned char> listed((size_t)n_samp, 0);
    out->resize((size_t)n);
    for (i64 i = 0; i < n; ++i) {
        const T g = list[i];
        if (g < 0 || (u64)g >= n_samp)
            return fail(UTM_EINVAL, "%s, entry %lld: sample %lld not in [0,%llu)", what, (long long)i, (long long)g, (unsigned long long)n_samp);
        if (listed[(size_t)g]) return fail(UTM_EINVAL, "%s, entry %lld: sample %lld is listed twice", what, (long long)i, (long long)g);
        listed[(size_t)g] = 1;
        (*out)[(size_t)i] = (unsigned)g;
    }
    return UTM_OK;
}

extern "C" int utm_coverage_bound(utm_ctx *c, const int64_t *cand, int64_t n_cand, const int64_t *given, int64_t n_given, int64_t k,
                                  int32_t iters, uint32_t step0, uint32_t period, int64_t *hist_out, int64_t *bound_out,
                                  int32_t *best_iter_out, int64_t *n_live_out, uint32_t *const *lambda_out, double *pass_ms)
{
    CTX(c);
    if (depth_sharded(c))
        return fail(UTM_ESTATE, "the coverage bound needs the whole sample axis in one context without an exchange (this one holds samples "
                                "%u..%u of %u)", c->first, c->first + c->n_local, c->n_total);
    std::vector<unsigned> h_cand, h_given;
    if (!cand && n_cand == 0) {
        h_cand.resize(c->n_total);
        for (unsigned s = 0; s < c->n_total; ++s) h_cand[s] = s;
    } else {
        TRY(bound_list(cand, n_cand, c->n_total, "cand", &h_cand));
    }
    TRY(bound_list(given, n_given, c->n_total, "given", &h_given));
    const i64 n_c = (i64)h_cand.size();
    BoundArgs a;
    TRY(bound_args(n_c, k, iters, step0, period, hist_out, &a));
    if (lambda_out)
        for (size_t i = 0; i < c->chunks.size(); ++i)
            if (!lambda_out[i] && c->chunks[i].n_var) return fail(UTM_EINVAL, "lambda_out[%zu] is NULL", i);
    if (pass_ms) *pass_ms = 0.0;

    // Nothing of the context is read but the chunks' columns, and nothing of it is written: the lists, the live masks,
    // lambda, the sums and the history are this call's own.  The launches go on the context's stream.
    const u64 words = std::max<u64>(c->col_words, 1);
    Scratch<unsigned> d_cand, d_given, d_picked, d_lambda;
    Scratch<u64> d_live, d_single, d_sums, d_misc;  // misc: [0], [1] the constant term of even / odd iterations, [2] n_live
    Scratch<i64> d_hist;
    u64 wp_max = 0;
    for (const Chunk &ch : c->chunks) wp_max = std::max(wp_max, ch.wp);
    HIP_TRY(d_cand.alloc((size_t)std::max<i64>(n_c, 1)));
    HIP_TRY(d_given.alloc(std::max<size_t>(h_given.size(), 1)));
    HIP_TRY(d_picked.alloc((size_t)std::max<i64>(a.kk, 1)));
    HIP_TRY(d_lambda.alloc((size_t)words * 64));
    HIP_TRY(d_live.alloc((size_t)words));
    HIP_TRY(d_single.alloc((size_t)std::max<u64>(wp_max, 1)));
    HIP_TRY(d_sums.alloc((size_t)std::max<i64>(n_c, 1)));
    HIP_TRY(d_misc.alloc(4));
    HIP_TRY(d_hist.alloc((size_t)iters));
    if (n_c) HIP_TRY(hipMemcpyAsync(d_cand.p, h_cand.data(), (size_t)n_c * 4, hipMemcpyHostToDevice, c->stream));
    if (!h_given.empty()) HIP_TRY(hipMemcpyAsync(d_given.p, h_given.data(), h_given.size() * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(d_sums.p, 0, (size_t)std::max<i64>(n_c, 1) * 8, c->stream));
    HIP_TRY(hipMemsetAsync(d_misc.p, 0, 4 * 8, c->stream));
    struct Events {
        hipEvent_t e0 = nullptr, e1 = nullptr;
        ~Events() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
    } ev;
    if (pass_ms) {
        HIP_TRY(hipEventCreate(&ev.e0));
        HIP_TRY(hipEventCreate(&ev.e1));
        HIP_TRY(hipEventRecord(ev.e0, c->stream));
    }
    for (const Chunk &ch : c->chunks) {
        if (ch.n_var == 0) continue;
        const u64 tiles = (ch.wp + UTM_SWAP_TILE_WORDS - 1) / UTM_SWAP_TILE_WORDS;
        hipLaunchKernelGGL(k_swap_masks, dim3((unsigned)tiles), dim3(256), 0, c->stream, (const u64 *)ch.cols, ch.wp, ch.n_var, (const unsigned *)d_given.p,
                           (unsigned)h_given.size(), d_single.p, d_live.p + ch.off);
        hipLaunchKernelGGL(k_bound_init, dim3((unsigned)((ch.wp * 16 + 255) / 256)), dim3(256), 0, c->stream, (const u64 *)(d_live.p + ch.off), ch.wp,
                           d_lambda.p + ch.off * 64, d_misc.p + 2);
        HIP_TRY(hipGetLastError());
    }
    // the T iterations, enqueued without a host round trip
    BoundTimers tm;
    tm.on = (c->flags & UTM_FLAG_PROFILE_EVENTS) != 0;
    hipEvent_t es = nullptr, ee = nullptr;
    const unsigned n_groups = (unsigned)((n_c + UTM_BOUND_GROUP - 1) / UTM_BOUND_GROUP);
    for (int32_t t = 0; t < iters; ++t) {
        if (n_c)
            for (const Chunk &ch : c->chunks) {
                if (ch.n_var == 0) continue;
                // runs: as long as UTM_BOUND_RUN allows while the grid keeps about 8 workgroups per CU
                const u64 tiles = ch.wp / UTM_BOUND_TILE_WORDS;
                const unsigned run = (unsigned)std::min<u64>(UTM_BOUND_RUN, std::max<u64>(1, tiles * n_groups / 2048));
                const u64 n_runs = (tiles + run - 1) / run;
                tm.pair(0, &es, &ee);
                hipExtLaunchKernelGGL(k_bound_sums, dim3((unsigned)(n_runs * n_groups)), dim3(UTM_BOUND_THREADS), 0, c->stream, es, ee, 0, (const u64 *)ch.cols, ch.wp,
                                   (const unsigned *)(d_lambda.p + ch.off * 64), (const unsigned *)d_cand.p, (unsigned)n_c, d_sums.p, n_groups, run);
            }
        tm.pair(1, &es, &ee);
        hipExtLaunchKernelGGL(k_bound_pick, dim3(1), dim3(UTM_BOUND_PICK_THREADS), 0, c->stream, es, ee, 0, d_sums.p, (const unsigned *)d_cand.p, (unsigned)n_c,
                           (unsigned)a.kk, d_picked.p, d_misc.p, d_hist.p, (unsigned)t);
        const unsigned eta = bound_eta(a.step0, a.period, (unsigned)t);
        for (const Chunk &ch : c->chunks) {
            if (ch.n_var == 0) continue;
            tm.pair(2, &es, &ee);
            hipExtLaunchKernelGGL(k_bound_update, dim3((unsigned)((ch.wp + 255) / 256)), dim3(256), 0, c->stream, es, ee, 0, (const u64 *)ch.cols, ch.wp,
                               (const u64 *)(d_live.p + ch.off), (const unsigned *)d_picked.p, (unsigned)a.kk, eta, d_lambda.p + ch.off * 64,
                               d_misc.p + ((t + 1) & 1));
        }
        HIP_TRY(hipGetLastError());
    }
    if (pass_ms) HIP_TRY(hipEventRecord(ev.e1, c->stream));
    // into memory of this call first: the outputs stay untouched if a pass fails
    std::vector<i64> h_hist((size_t)iters);
    u64 h_misc[4];
    HIP_TRY(hipMemcpyAsync(h_misc, d_misc.p, sizeof h_misc, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(copy_sync(c, h_hist.data(), d_hist.p, (size_t)iters * 8, hipMemcpyDeviceToHost));
    if (lambda_out)
        for (const Chunk &ch : c->chunks)
            if (ch.n_var) HIP_TRY(copy_sync(c, lambda_out[ch.index], d_lambda.p + ch.off * 64, (size_t)ch.n_var * 4, hipMemcpyDeviceToHost));
    if (pass_ms) {
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, ev.e0, ev.e1));
        *pass_ms = ms;
    }
    c->bound_ms[0] = c->bound_ms[1] = c->bound_ms[2] = 0.0;
    for (size_t i = 0; i < tm.kind.size(); ++i) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, tm.ev[2 * i], tm.ev[2 * i + 1]) == hipSuccess) c->bound_ms[tm.kind[i]] += ms;
    }
    std::copy(h_hist.begin(), h_hist.end(), hist_out);
    bound_from_hist(h_hist.data(), iters, (i64)h_misc[2], bound_out, best_iter_out, n_live_out);
    return UTM_OK;
}

// The last utm_coverage_bound call's summed HIP-event times of k_bound_sums, k_bound_pick and k_bound_update, in ms; zeros
// unless the context was created with UTM_FLAG_PROFILE_EVENTS.
extern "C" int utm_coverage_bound_times(utm_ctx *c, double *ms_out)
{
    if (!c || !ms_out) return fail(UTM_EINVAL, "NULL argument");
    std::copy(c->bound_ms, c->bound_ms + 3, ms_out);
    return UTM_OK;
}

// The same arithmetic built for the CPU: one chunk's columns (cols[s * wp + w], n_var <= 64 * wp variants, n_samp columns).
// cand == NULL with n_cand == 0: every sample, in index order.  lambda_out: n_var values, 0 where a variant is not live.
// Needs no GPU.
extern "C" int utm_coverage_bound_host(const uint64_t *cols, uint64_t wp, uint64_t n_var, uint32_t n_samp, const uint32_t *cand, uint64_t n_cand,
                                       const uint32_t *given, uint64_t n_given, int64_t k, int32_t iters, uint32_t step0, uint32_t period,
                                       int64_t *hist_out, int64_t *bound_out, int32_t *best_iter_out, int64_t *n_live_out, uint32_t *lambda_out)
{
    if (n_var > wp * 64 || (!cols && n_var && n_samp)) return fail(UTM_EINVAL, "%llu variants in %llu words", (unsigned long long)n_var, (unsigned long long)wp);
    if (n_cand > n_samp || n_given > n_samp) return fail(UTM_EINVAL, "a list longer than the %u samples", n_samp);
    std::vector<unsigned> h_cand, h_given;
    if (!cand && n_cand == 0) {
        h_cand.resize(n_samp);
        for (unsigned s = 0; s < n_samp; ++s) h_cand[s] = s;
    } else {
        std::vector<i64> wide(cand ? cand : nullptr, cand ? cand + n_cand : nullptr);
        TRY(bound_list(cand ? wide.data() : (const i64 *)nullptr, (i64)n_cand, n_samp, "cand", &h_cand));
    }
    {
        std::vector<i64> wide(given ? given : nullptr, given ? given + n_given : nullptr);
        TRY(bound_list(given ? wide.data() : (const i64 *)nullptr, (i64)n_given, n_samp, "given", &h_given));
    }
    const u64 n_c = h_cand.size();
    BoundArgs a;
    TRY(bound_args((i64)n_c, k, iters, step0, period, hist_out, &a));
    const u64 *q = (const u64 *)cols;
    const u64 words = (n_var + 63) / 64;
    std::vector<u64> live(words);
    i64 n_live = 0;
    for (u64 w = 0; w < words; ++w) {
        u64 once = 0, twice = 0;
        for (unsigned g : h_given) swap_count(q[(u64)g * wp + w], once, twice);
        live[w] = swap_uncovered(once, swap_valid(w, n_var));
        n_live += __builtin_popcountll(live[w]);
    }
    std::vector<unsigned> lambda((size_t)n_var, 0);
    for (u64 v = 0; v < n_var; ++v)
        if (live[v >> 6] >> (v & 63) & 1) lambda[v] = UTM_BOUND_Q;
    std::vector<i64> hist((size_t)iters), s((size_t)n_c);
    std::vector<unsigned> order((size_t)n_c), cnt((size_t)n_var);
    i64 konst = 0;  // sum over the live variants of Q - lambda
    for (int32_t t = 0; t < iters; ++t) {
        for (u64 j = 0; j < n_c; ++j) {
            i64 sum = 0;
            const u64 *col = q + (u64)h_cand[j] * wp;
            for (u64 w = 0; w < words; ++w)
                for (u64 b = col[w] & live[w]; b; b &= b - 1) sum += lambda[w * 64 + (u64)__builtin_ctzll(b)];
            s[j] = sum;
        }
        for (u64 j = 0; j < n_c; ++j) order[j] = (unsigned)j;
        std::stable_sort(order.begin(), order.end(), [&](unsigned x, unsigned y) { return s[x] > s[y]; });  // ties: the smaller position first
        i64 L = konst;
        std::fill(cnt.begin(), cnt.end(), 0u);
        for (i64 r = 0; r < a.kk; ++r) {
            L += s[order[(size_t)r]];
            const u64 *col = q + (u64)h_cand[order[(size_t)r]] * wp;
            for (u64 w = 0; w < words; ++w)
                for (u64 b = col[w] & live[w]; b; b &= b - 1) cnt[w * 64 + (u64)__builtin_ctzll(b)] += 1;
        }
        hist[(size_t)t] = L;
        const unsigned eta = bound_eta(a.step0, a.period, (unsigned)t);
        konst = 0;
        for (u64 v = 0; v < n_var; ++v) {
            if (!(live[v >> 6] >> (v & 63) & 1)) continue;
            lambda[v] = bound_step(lambda[v], eta, (i64)cnt[v]);
            konst += (i64)(UTM_BOUND_Q - lambda[v]);
        }
    }
    std::copy(hist.begin(), hist.end(), hist_out);
    bound_from_hist(hist.data(), iters, n_live, bound_out, best_iter_out, n_live_out);
    if (lambda_out) std::copy(lambda.begin(), lambda.end(), lambda_out);
    return UTM_OK;
}
