// Replicated selection: utm_multi_select (k_multi_keep / k_multi_init once, then k_multi_score + k_multi_pick +
// k_multi_apply per iteration, the whole loop enqueued without a host round trip per iteration) and the CPU build of the
// same arithmetic.  Part of the one translation unit utmos_hip.hip (included there, in order); not a stand-alone header.
#pragma once

#define UTM_MULTI_TARGET_WGS 8192  // workgroups of a k_multi_score launch, about (as UTM_SWAP_TARGET_WGS)
#define UTM_MULTI_CHECK_EVERY 32   // iterations between two looks of the host at the number of running replicates

static int multi_check_states(const uint8_t *state, u64 n_rep, u64 n)
{
    for (u64 i = 0; i < n_rep * n; ++i)
        if (state[i] > 2) return fail(UTM_EINVAL, "replicate %llu, sample %llu: state %u is not 0, 1 or 2", (unsigned long long)(i / n),
                                      (unsigned long long)(i % n), state[i]);
    return UTM_OK;
}

// What the reference offers instead: nothing -- a caller would filter the VCF per replicate, convert and select B times.
extern "C" int utm_multi_select(utm_ctx *c, uint32_t n_rep, const uint8_t *state, const uint64_t *const *keep, uint64_t seed,
                                uint64_t keep_threshold, int64_t k, int32_t *order_out, int64_t *new_out, int64_t *kept_out, int64_t *n_done,
                                double *pass_ms)
{
    CTX(c);
    if (n_rep < 1 || n_rep > UTM_MULTI_MAX_REP) return fail(UTM_EINVAL, "%u replicates: not in 1..%d", n_rep, UTM_MULTI_MAX_REP);
    if (k < 0) return fail(UTM_EINVAL, "k = %lld", (long long)k);
    if (!state || !order_out || !new_out || !kept_out || !n_done) return fail(UTM_EINVAL, "NULL argument");
    const u64 n = c->n_total, B = n_rep;
    TRY(multi_check_states(state, B, n));
    if (keep)
        for (size_t i = 0; i < c->chunks.size(); ++i)
            if (!keep[i]) return fail(UTM_EINVAL, "keep[%zu] is NULL", i);
    if (depth_sharded(c))
        return fail(UTM_ESTATE, "a replicated selection needs the whole sample axis in one context without an exchange (this one holds "
                                "samples %u..%u of %u)", c->first, c->first + c->n_local, c->n_total);

    // Nothing of the context is read but the chunks' columns, and nothing of it is written: the states, the live masks, the
    // scores, the rows and the events are this call's own.  The launches go on the context's stream.
    const i64 iters = std::min<i64>(k, (i64)n);  // a replicate cannot make more rows than it has samples
    const unsigned row_blocks = (unsigned)((B + 63) / 64), rb = row_blocks * 64;
    const unsigned cand_blocks = (unsigned)((n + UTM_SWAP_T - 1) / UTM_SWAP_T);
    std::vector<unsigned> used_off(B + 1, 0), used_idx;
    for (u64 b = 0; b < B; ++b) {
        for (u64 s = 0; s < n; ++s)
            if (state[b * n + s] == 0) used_idx.push_back((unsigned)s);
        used_off[b + 1] = (unsigned)used_idx.size();
    }
    Scratch<u64> d_live, d_scores, d_kept;
    Scratch<unsigned char> d_state, d_done;
    Scratch<unsigned> d_used_off, d_used_idx;
    Scratch<int> d_winner, d_order;
    Scratch<i64> d_gain, d_rows;  // d_rows: rows[B], tot[B]
    Scratch<MultiCtl> d_ctl;
    if (d_live.alloc((size_t)(B * std::max<u64>(c->col_words, 1))) != hipSuccess || d_scores.alloc((size_t)std::max<u64>(n, 1) * rb) != hipSuccess) {
        (void)hipGetLastError();
        return fail(UTM_ENOMEM, "no room for %u live masks of %llu words and %u x %llu scores", n_rep, (unsigned long long)c->col_words, n_rep,
                    (unsigned long long)n);
    }
    HIP_TRY(d_kept.alloc(B));
    HIP_TRY(d_state.alloc((size_t)(B * n)));
    HIP_TRY(d_done.alloc(B));
    HIP_TRY(d_used_off.alloc(B + 1));
    HIP_TRY(d_used_idx.alloc(std::max<size_t>(used_idx.size(), 1)));
    HIP_TRY(d_winner.alloc(B));
    HIP_TRY(d_order.alloc((size_t)std::max<i64>(B * iters, 1)));
    HIP_TRY(d_gain.alloc((size_t)std::max<i64>(B * iters, 1)));
    HIP_TRY(d_rows.alloc(2 * B));
    HIP_TRY(d_ctl.alloc(1));
    const MultiCtl ctl0{(int)B, 0};
    HIP_TRY(hipMemsetAsync(d_live.p, 0, (size_t)(B * std::max<u64>(c->col_words, 1)) * 8, c->stream));
    HIP_TRY(hipMemsetAsync(d_scores.p, 0, (size_t)std::max<u64>(n, 1) * rb * 8, c->stream));
    HIP_TRY(hipMemsetAsync(d_kept.p, 0, B * 8, c->stream));
    HIP_TRY(hipMemsetAsync(d_done.p, 0, B, c->stream));
    HIP_TRY(hipMemsetAsync(d_winner.p, 0xFF, B * 4, c->stream));
    HIP_TRY(hipMemsetAsync(d_order.p, 0xFF, (size_t)std::max<i64>(B * iters, 1) * 4, c->stream));
    HIP_TRY(hipMemsetAsync(d_gain.p, 0, (size_t)std::max<i64>(B * iters, 1) * 8, c->stream));
    HIP_TRY(hipMemsetAsync(d_rows.p, 0, 2 * B * 8, c->stream));
    HIP_TRY(hipMemcpyAsync(d_state.p, state, (size_t)(B * n), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(d_used_off.p, used_off.data(), (B + 1) * 4, hipMemcpyHostToDevice, c->stream));
    if (!used_idx.empty()) HIP_TRY(hipMemcpyAsync(d_used_idx.p, used_idx.data(), used_idx.size() * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(d_ctl.p, &ctl0, sizeof ctl0, hipMemcpyHostToDevice, c->stream));
    struct Events {
        hipEvent_t e0 = nullptr, e1 = nullptr;
        ~Events() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
    } ev;
    if (pass_ms) {
        HIP_TRY(hipEventCreate(&ev.e0));
        HIP_TRY(hipEventCreate(&ev.e1));
        HIP_TRY(hipEventRecord(ev.e0, c->stream));
    }

    // the masks: a chunk's B live rows lie at B x (the chunk's word offset in a whole column)
    u64 first_var = 0;
    for (size_t i = 0; i < c->chunks.size(); ++i) {
        const Chunk &ch = c->chunks[i];
        u64 *live = d_live.p + B * ch.off;
        const u64 words = (ch.n_var + 63) / 64;
        if (words) {
            if (keep)
                HIP_TRY(hipMemcpy2DAsync(live, ch.wp * 8, keep[i], words * 8, words * 8, B, hipMemcpyHostToDevice, c->stream));
            else
                hipLaunchKernelGGL(k_multi_keep, dim3((unsigned)((words + 255) / 256), n_rep), dim3(256), 0, c->stream, live, ch.wp, words, ch.n_var, first_var,
                                   (u64)seed, (u64)keep_threshold);
            const u64 tiles = (ch.wp + UTM_SWAP_TILE_WORDS - 1) / UTM_SWAP_TILE_WORDS;
            hipLaunchKernelGGL(k_multi_init, dim3((unsigned)tiles, n_rep), dim3(256), 0, c->stream, (const u64 *)ch.cols, ch.wp, ch.n_var, live,
                               (const unsigned *)d_used_off.p, (const unsigned *)d_used_idx.p, d_kept.p);
            HIP_TRY(hipGetLastError());
        }
        first_var += ch.n_var;
    }

    MultiPick pick;
    pick.scores = d_scores.p;
    pick.state = d_state.p;
    pick.done = d_done.p;
    pick.winner = d_winner.p;
    pick.order = d_order.p;
    pick.gain = d_gain.p;
    pick.rows = d_rows.p;
    pick.tot = d_rows.p + B;
    pick.kept = d_kept.p;
    pick.ctl = d_ctl.p;
    pick.n = (unsigned)n;
    pick.rb = rb;
    pick.k = iters;
    for (i64 it = 0; it < iters; ++it) {
        for (const Chunk &ch : c->chunks) {
            if (ch.n_var == 0) continue;
            const u64 tiles = (ch.wp + UTM_SWAP_TILE_WORDS - 1) / UTM_SWAP_TILE_WORDS;
            u64 groups = std::max<u64>(1, UTM_MULTI_TARGET_WGS / ((u64)cand_blocks * row_blocks));
            groups = std::max(groups, (tiles + UTM_SWAP_MAX_TILES_PER_WG - 1) / UTM_SWAP_MAX_TILES_PER_WG);  // (an int32 accumulator per lane)
            groups = std::min(groups, tiles);
            hipLaunchKernelGGL(k_multi_score, dim3((unsigned)groups, cand_blocks, row_blocks), dim3(256), 0, c->stream, (const u64 *)ch.cols, ch.wp,
                               (unsigned)n, (const u64 *)(d_live.p + B * ch.off), n_rep, (const unsigned char *)d_done.p, (const MultiCtl *)d_ctl.p,
                               d_scores.p, rb);
        }
        hipLaunchKernelGGL(k_multi_pick, dim3(n_rep), dim3(256), 0, c->stream, pick);
        if (it + 1 < iters)
            for (const Chunk &ch : c->chunks) {
                if (ch.n_var == 0) continue;
                const u64 tiles = (ch.wp + UTM_SWAP_TILE_WORDS - 1) / UTM_SWAP_TILE_WORDS;
                hipLaunchKernelGGL(k_multi_apply, dim3((unsigned)tiles, n_rep), dim3(256), 0, c->stream, (const u64 *)ch.cols, ch.wp, d_live.p + B * ch.off,
                                   (const int *)d_winner.p, (const MultiCtl *)d_ctl.p);
            }
        HIP_TRY(hipGetLastError());
        if ((it + 1) % UTM_MULTI_CHECK_EVERY == 0 && it + 1 < iters) {  // every replicate has ended: the rest would be empty launches
            MultiCtl now;
            HIP_TRY(copy_sync(c, &now, d_ctl.p, sizeof now, hipMemcpyDeviceToHost));
            if (now.left == 0) break;
        }
    }
    if (pass_ms) HIP_TRY(hipEventRecord(ev.e1, c->stream));

    // into memory of this call first: the outputs stay untouched if a pass fails
    std::vector<int> h_order((size_t)(B * iters));
    std::vector<i64> h_gain((size_t)(B * iters)), h_rows(2 * B), h_kept(B);
    if (B * iters) {
        HIP_TRY(hipMemcpyAsync(h_order.data(), d_order.p, (size_t)(B * iters) * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(h_gain.data(), d_gain.p, (size_t)(B * iters) * 8, hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(hipMemcpyAsync(h_rows.data(), d_rows.p, 2 * B * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(copy_sync(c, h_kept.data(), d_kept.p, B * 8, hipMemcpyDeviceToHost));
    if (pass_ms) {
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, ev.e0, ev.e1));
        *pass_ms = ms;
    }
    for (u64 b = 0; b < B; ++b) {
        for (i64 i = 0; i < k; ++i) {
            order_out[b * (u64)k + i] = i < iters ? h_order[b * iters + i] : -1;
            new_out[b * (u64)k + i] = i < iters ? h_gain[b * iters + i] : 0;
        }
        kept_out[b] = h_kept[b];
        n_done[b] = h_rows[b];
    }
    return UTM_OK;
}

// The hashed mask of one replicate on the host: variants first_var_global .. + n_var, ceil(n_var / 64) words.
extern "C" int utm_multi_keep_host(uint64_t seed, uint32_t rep, uint64_t first_var_global, uint64_t n_var, uint64_t keep_threshold, uint64_t *words)
{
    if (n_var && !words) return fail(UTM_EINVAL, "words is NULL");
    for (u64 w = 0; w * 64 < n_var; ++w) {
        const u64 left = n_var - w * 64;
        words[w] = multi_keep_word(seed, rep, first_var_global + w * 64, left < 64 ? (unsigned)left : 64u, keep_threshold);
    }
    return UTM_OK;
}

// The kernels' arithmetic built for the CPU, replicate by replicate: cols[s * wp + w] of ONE chunk holding n_var <= 64 * wp
// variants of n_samp samples, state[n_rep * n_samp], keep[n_rep * ceil(n_var / 64)]; the outputs of utm_multi_select.  Needs
// no GPU.
extern "C" int utm_multi_select_host(const uint64_t *cols, uint64_t wp, uint64_t n_var, uint32_t n_samp, uint32_t n_rep, const uint8_t *state,
                                     const uint64_t *keep, int64_t k, int32_t *order_out, int64_t *new_out, int64_t *kept_out, int64_t *n_done)
{
    if (n_rep < 1 || n_rep > UTM_MULTI_MAX_REP) return fail(UTM_EINVAL, "%u replicates: not in 1..%d", n_rep, UTM_MULTI_MAX_REP);
    if (k < 0) return fail(UTM_EINVAL, "k = %lld", (long long)k);
    if (!state || !order_out || !new_out || !kept_out || !n_done || (n_var && (!keep || !cols))) return fail(UTM_EINVAL, "NULL argument");
    if (n_var > wp * 64) return fail(UTM_EINVAL, "%llu variants in %llu words", (unsigned long long)n_var, (unsigned long long)wp);
    const u64 n = n_samp, words = (n_var + 63) / 64;
    TRY(multi_check_states(state, n_rep, n));
    const u64 *q = (const u64 *)cols;
    std::vector<int32_t> order((size_t)n_rep * k, -1);
    std::vector<int64_t> gain((size_t)n_rep * k, 0), kept(n_rep, 0), rows(n_rep, 0);
    std::vector<u64> live(words);
    std::vector<i64> score(n);
    std::vector<unsigned char> st(n);
    for (u64 b = 0; b < n_rep; ++b) {
        std::copy(state + b * n, state + (b + 1) * n, st.begin());
        // k_multi_init
        for (u64 w = 0; w < words; ++w) {
            const u64 kw = keep[b * words + w] & swap_valid(w, n_var);
            kept[b] += __builtin_popcountll(kw);
            u64 used_or = 0;
            for (u64 s = 0; s < n; ++s)
                if (st[s] == 0) used_or |= q[s * wp + w];
            live[w] = multi_live(kw, ~0ull, used_or);
        }
        i64 tot = 0;
        while (rows[b] < k) {
            // k_multi_score
            std::fill(score.begin(), score.end(), 0);
            for (u64 w = 0; w < words; ++w) {
                if (!live[w]) continue;
                for (u64 t = 0; t < n; ++t) score[t] += swap_pair(live[w], q[t * wp + w]);
            }
            // k_multi_pick
            i64 best = 0, best_idx = -1;
            for (u64 s = 0; s < n; ++s)
                if (st[s] == 1 && multi_better(score[s], (i64)s, best, best_idx)) {
                    best = score[s];
                    best_idx = (i64)s;
                }
            if (best_idx < 0 || best == 0) break;
            order[b * (u64)k + rows[b]] = (int32_t)best_idx;
            gain[b * (u64)k + rows[b]] = best;
            ++rows[b];
            tot += best;
            st[best_idx] = 0;
            if (tot >= kept[b]) break;
            // k_multi_apply
            for (u64 w = 0; w < words; ++w) live[w] &= ~q[(u64)best_idx * wp + w];
        }
    }
    std::copy(order.begin(), order.end(), order_out);
    std::copy(gain.begin(), gain.end(), new_out);
    std::copy(kept.begin(), kept.end(), kept_out);
    std::copy(rows.begin(), rows.end(), n_done);
    return UTM_OK;
}
