// Fixed orders: utm_apply_order (one k_order_curve launch per chunk; depth M > 1: one k_depth_apply per listed sample and
// chunk) and the CPU build of its loop.
// Part of the one translation unit utmos_hip.hip (included there, in order); not a stand-alone header.
#pragma once

extern "C" int utm_apply_order(utm_ctx *c, const int64_t *global_idx, int64_t n, int64_t *new_out, int64_t *n_done)
{
    CTX(c);
    if (!n_done || n < 0 || (n > 0 && (!global_idx || !new_out))) return fail(UTM_EINVAL, "bad arguments");
    *n_done = 0;
    if (c->chunks.empty()) return fail(UTM_ESTATE, "no chunks");
    if (c->n_local != c->n_total || c->n_ranks != 1 || c->comm || c->p2p || mailbox_exchange(c))
        return fail(UTM_ESTATE, "a fixed order needs the whole sample axis in one context without an exchange (this one holds samples "
                                "%u..%u of %u)", c->first, c->first + c->n_local, c->n_total);
    TRY(ensure_prepared(c));
    // the states as the loop left them (winners of earlier utm_run calls are used; h_state only has the initial ones)
    std::vector<unsigned char> state(c->n_total);
    HIP_TRY(copy_sync(c, state.data(), c->d_state, c->n_total, hipMemcpyDeviceToHost));
    if (n > (i64)c->n_total) return fail(UTM_EINVAL, "%lld samples listed, the matrix has %u", (long long)n, c->n_total);
    std::vector<unsigned> order((size_t)n);
    {
        std::vector<unsigned char> listed(c->n_total, 0);
        for (i64 i = 0; i < n; ++i) {
            const i64 g = global_idx[i];
            if (g < 0 || g >= (i64)c->n_total) return fail(UTM_EINVAL, "entry %lld: sample %lld not in [0,%u)", (long long)i, (long long)g, c->n_total);
            if (listed[g]) return fail(UTM_EINVAL, "entry %lld: sample %lld is listed twice", (long long)i, (long long)g);
            if (state[g] == 0) return fail(UTM_EINVAL, "entry %lld: sample %lld is already used", (long long)i, (long long)g);
            listed[g] = 1;
            order[(size_t)i] = (unsigned)g;
        }
    }
    const bool deep = c->depth > 1;  // every listed column goes through k_depth_apply, gains = units
    const i64 f_max = (i64)c->n_var_total * c->depth;
    if (n == 0 || c->captured_seen >= f_max) return UTM_OK;  // nothing listed / nothing left to capture

    Scratch<unsigned> d_order;
    Scratch<u64> d_counts;
    HIP_TRY(d_order.alloc((size_t)n));
    HIP_TRY(d_counts.alloc((size_t)n));
    HIP_TRY(hipMemcpyAsync(d_order.p, order.data(), (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(d_counts.p, 0, (size_t)n * 8, c->stream));
    Scratch<u64> d_sat;  // depth: variants that became saturated, per listed sample
    if (deep) {
        HIP_TRY(d_sat.alloc((size_t)n));
        HIP_TRY(hipMemsetAsync(d_sat.p, 0, (size_t)n * 8, c->stream));
    }
    HIP_TRY(hipEventRecord(c->ev_loop0, c->stream));
    TRY(flush_pending(c));  // the last winner's column may still be waiting for the next scoring launch
    const bool use_nt = c->tune.nt_loads >= 0 ? c->tune.nt_loads != 0 : (u64)n * c->col_words * 8 > ((u64)c->tune.nt_min_mb << 20);
    for (auto &ch : c->chunks) {
        const dim3 grid((unsigned)((ch.wp + UTM_ORDER_TILE_WORDS - 1) / UTM_ORDER_TILE_WORDS));
        if (deep)
            for (i64 i = 0; i < n; ++i)
                launch_depth_apply(c, ch, ch.cols + (u64)order[(size_t)i] * ch.wp, d_counts.p + i, d_sat.p + i, false);
        else if (use_nt)
            hipLaunchKernelGGL(k_order_curve<true>, grid, dim3(256), 0, c->stream, (const u64 *)ch.cols, ch.covered, ch.wp,
                               (const unsigned *)d_order.p, (unsigned)n, d_counts.p);
        else
            hipLaunchKernelGGL(k_order_curve<false>, grid, dim3(256), 0, c->stream, (const u64 *)ch.cols, ch.covered, ch.wp,
                               (const unsigned *)d_order.p, (unsigned)n, d_counts.p);
        // AF contexts keep a pair of covered buffers that swap roles: both hold the new mask
        if (ch.covered_alt) HIP_TRY(hipMemcpyAsync(ch.covered_alt, ch.covered, ch.wp * 8, hipMemcpyDeviceToDevice, c->stream));
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->ev_loop1, c->stream));
    std::vector<u64> counts((size_t)n);
    HIP_TRY(copy_sync(c, counts.data(), d_counts.p, (size_t)n * 8, hipMemcpyDeviceToHost));
    std::vector<i64> at_depth;
    if (deep) {
        // the running number of saturated variants after each row (columns behind the last row found nothing to add)
        std::vector<u64> sat((size_t)n);
        u64 running = 0;
        HIP_TRY(copy_sync(c, sat.data(), d_sat.p, (size_t)n * 8, hipMemcpyDeviceToHost));
        HIP_TRY(copy_sync(c, &running, c->d_depth_acc + 1, 8, hipMemcpyDeviceToHost));
        for (i64 i = 0; i < n; ++i) at_depth.push_back((i64)(running += sat[(size_t)i]));
        HIP_TRY(copy_sync(c, c->d_depth_acc + 1, &running, 8, hipMemcpyHostToDevice));
        if (c->flags & UTM_FLAG_PROFILE_EVENTS) TRY(collect_depth_times(c));
    }

    // Rows end after the one that captures the last variant.  The columns listed behind it were ORed into a mask that was
    // complete already, so covered is what the rows alone make it; those samples keep their states.
    i64 tot = c->captured_seen, rows = 0;
    std::vector<i64> idx;
    while (rows < n) {
        const unsigned g = order[(size_t)rows];
        new_out[rows] = (i64)counts[(size_t)rows];
        tot += new_out[rows];
        state[g] = 0;
        idx.push_back((i64)g);
        rows += 1;
        if (tot >= f_max) break;
    }
    const i64 iter0 = c->iter;
    HIP_TRY(hipMemcpyAsync(c->d_res_idx + iter0, idx.data(), (size_t)rows * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->d_res_new + iter0, new_out, (size_t)rows * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(c->d_res_score + iter0, 0, (size_t)rows * 8, c->stream));
    if (deep) HIP_TRY(hipMemcpyAsync(c->d_res_sat + iter0, at_depth.data(), (size_t)rows * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));  // (idx and new_out are the caller's / this call's memory)
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, c->ev_loop0, c->ev_loop1));
    c->loop_ms = ms;  // (utm_stats.loop_ms: the pass, as for a utm_run)
    c->algo_bytes += deep ? (i64)n * (2 * c->depth_planes + 3) * (i64)c->col_words * 8 : (i64)((u64)n + 2) * (i64)c->col_words * 8;
    // Everything cached about scores goes: counts by position in act[], AF sums and records, the decremental copy's
    // bookkeeping, the persistent loop's words -- the path of utm_reset, with covered, the rows and the total kept.
    TRY(reset_loop_state(c, state.data(), /*restart=*/false, iter0 + rows, tot));
    *n_done = rows;
    return UTM_OK;
}

// The kernel's walk built for the CPU: one chunk's columns (cols[s * wp + w]), its covered words (updated in place), a
// list of n column indices; counts[i] += what column order[i] newly covers.  Needs no GPU.
extern "C" int utm_order_curve_host(const uint64_t *cols, uint64_t wp, uint64_t *covered, const uint32_t *order, uint64_t n,
                                    uint64_t *counts)
{
    if (!cols || !covered || (n && (!order || !counts))) return fail(UTM_EINVAL, "NULL argument");
    for (u64 w = 0; w < wp; ++w) {
        u64 cov = covered[w];
        for (u64 i = 0; i < n; ++i) counts[i] += order_word(cols[(u64)order[i] * wp + w], cov);
        covered[w] = cov;
    }
    return UTM_OK;
}
