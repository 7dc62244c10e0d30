// DEFLATE context (utm_deflate_*): host side of deflate.hip.h.  One raw-deflate stream is compressed in batches of
// whole 64 KiB segments (the last batch of a stream may end with a shorter one); the caller adds the zlib header and
// the Adler-32 trailer that utm_deflate_adler combines from the segments' sums.
//
// One pinned staging buffer and two slots (host_batch.hip.h), each with its own device buffers and pinned output:
// utm_deflate_push returns once its batch has reached the device and the kernels are queued, so the caller fills the
// staging again while the GPU compresses; utm_deflate_pull collects the oldest batch's bytes.
#pragma once

struct DefSlot : BatchSlot<7> {  // events: H2D (0-1), chain + match (1-2), parse (2-3), encode + scan + gather (3-4), D2H (5-6)
    Scratch<uint8_t> d_in, d_seg, d_out;
    Pinned<uint8_t> h_out;
    Scratch<uint16_t> d_prev;
    Scratch<uint32_t> d_match, d_tok, d_ntok, d_sizes, d_offs, d_adler;
    Pinned<uint32_t> h_info;  // [0] output bytes of the batch, then (sum, weighted sum) per segment
    u64 n = 0;
    uint32_t nseg = 0;
    bool first = false;
};

struct utm_deflate : SlotPair<DefSlot> {
    int device = 0, level = 5;
    u64 batch = 0;
    uint32_t max_seg = 0;
    Pinned<uint8_t> h_stage;
    bool fresh = true;              // the next push starts a stream
    uint32_t a = 1, b = 0;          // Adler-32 halves of the pulled batches of the current stream
    double ms[4] = {0, 0, 0, 0};    // H2D, kernels, D2H, of the kernels the parse
    ~utm_deflate() { idle(device); }
};

static u64 def_bound(u64 n) { return n + 15 * std::max<u64>(1, (n + DEF_SEG - 1) / DEF_SEG); }

// Running Adler-32 (a, b) followed by a segment of `len` bytes with sums (s1, s2) (deflate.hip.h, def_encode).
static void def_adler_add(uint32_t *a, uint32_t *b, u64 len, uint32_t s1, uint32_t s2)
{
    const u64 a0 = *a;
    *a = (uint32_t)((a0 + s1) % DEF_ADLER_MOD);
    *b = (uint32_t)((*b + (len % DEF_ADLER_MOD) * a0 + s2) % DEF_ADLER_MOD);
}

static int def_check_level(int level)
{
    if (level < 1 || level > 9) return fail(UTM_EINVAL, "level %d not in [1, 9]", level);
    return UTM_OK;
}

extern "C" int utm_deflate_bound(uint64_t n_bytes, uint64_t *bound)
{
    if (!bound) return fail(UTM_EINVAL, "bound is NULL");
    *bound = def_bound(n_bytes);
    return UTM_OK;
}

extern "C" int utm_deflate_create(int device, uint64_t batch_bytes, int level, utm_deflate **out)
{
    if (!out) return fail(UTM_EINVAL, "out is NULL");
    *out = nullptr;
    TRY(def_check_level(level));
    if (batch_bytes == 0 || batch_bytes > UTM_DEFLATE_MAX_BATCH)
        return fail(UTM_EINVAL, "batch_bytes %llu not in [1, 2^30]", (unsigned long long)batch_bytes);
    TRY(open_device(device));
    std::unique_ptr<utm_deflate> p(new utm_deflate());
    p->device = device;
    p->level = level;
    p->max_seg = (uint32_t)((batch_bytes + DEF_SEG - 1) / DEF_SEG);
    p->batch = (u64)p->max_seg * DEF_SEG;
    const u64 nb = p->batch, ns = p->max_seg;
    TRY(p->h_stage.reserve(nb));
    for (DefSlot &s : p->slot) {
        TRY(s.open());
        TRY(s.d_in.reserve(nb + DEF_PAD));
        TRY(s.d_prev.reserve(nb));
        TRY(s.d_match.reserve(nb));
        TRY(s.d_tok.reserve(nb));
        TRY(s.d_seg.reserve(ns * DEF_SEG_OUT));
        TRY(s.d_out.reserve(def_bound(nb)));
        TRY(s.d_ntok.reserve(ns));
        TRY(s.d_sizes.reserve(ns));
        TRY(s.d_offs.reserve(ns + 1));
        TRY(s.d_adler.reserve(2 * ns));
        TRY(s.h_out.reserve(def_bound(nb)));
        TRY(s.h_info.reserve(1 + 2 * ns));
    }
    *out = p.release();
    return UTM_OK;
}

extern "C" int utm_deflate_destroy(utm_deflate *p)
{
    delete p;
    return UTM_OK;
}

extern "C" int utm_deflate_staging(utm_deflate *p, uint8_t **buf, uint64_t *cap)
{
    if (!p || !buf || !cap) return fail(UTM_EINVAL, "deflate, buf or cap is NULL");
    *buf = p->h_stage;
    *cap = p->batch;
    return UTM_OK;
}

extern "C" int utm_deflate_push(utm_deflate *p, const uint8_t *in, uint64_t n_bytes, uint32_t flags)
{
    BATCH_CTX(p, "deflate");
    if (flags & ~UTM_DEFLATE_LAST) return fail(UTM_EINVAL, "unknown flags 0x%x", flags);
    const bool last = flags & UTM_DEFLATE_LAST;
    if (n_bytes && !in) return fail(UTM_EINVAL, "in is NULL");
    if (n_bytes > p->batch) return fail(UTM_EINVAL, "a batch of %llu bytes (the context takes %llu)", (unsigned long long)n_bytes, (unsigned long long)p->batch);
    if (!last && n_bytes % DEF_SEG)
        return fail(UTM_EINVAL, "a batch of %llu bytes that is not the last must be a multiple of %u", (unsigned long long)n_bytes, DEF_SEG);
    DefSlot *s;
    TRY(p->free_slot("utm_deflate_pull", &s));
    if (n_bytes && in != p->h_stage) memcpy(p->h_stage, in, n_bytes);
    const uint32_t n = (uint32_t)n_bytes;
    const uint32_t nseg = last ? std::max<uint32_t>(1, (n + DEF_SEG - 1) / DEF_SEG) : n / DEF_SEG;
    HIP_TRY(hipEventRecord(s->ev[0], s->stream));
    if (n) HIP_TRY(hipMemcpyAsync(s->d_in, p->h_stage, n, hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipEventRecord(s->ev[1], s->stream));
    if (nseg) {
        k_deflate_chain<<<nseg, DEF_ROUND, 0, s->stream>>>(s->d_in, n, s->d_prev);
        k_deflate_match<<<dim3(DEF_SEG / DEF_THREADS, nseg), DEF_THREADS, 0, s->stream>>>(s->d_in, n, s->d_prev, s->d_match, p->level);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(s->ev[2], s->stream));
    if (nseg) k_deflate_parse<<<nseg, 64, 0, s->stream>>>(s->d_in, n, s->d_match, s->d_tok, s->d_ntok, p->level);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(s->ev[3], s->stream));
    if (nseg) {
        k_deflate_encode<<<nseg, DEF_THREADS, 0, s->stream>>>(s->d_in, n, s->d_tok, s->d_ntok, last ? (int)nseg - 1 : -1,
                                                              s->d_seg, s->d_sizes, s->d_adler);
        k_deflate_scan<<<1, DEF_THREADS, 0, s->stream>>>(s->d_sizes, nseg, s->d_offs);
        k_deflate_gather<<<nseg, DEF_THREADS, 0, s->stream>>>(s->d_seg, s->d_sizes, s->d_offs, s->d_out);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(s->h_info, s->d_offs + nseg, sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream));
        HIP_TRY(hipMemcpyAsync(s->h_info + 1, s->d_adler, 2 * nseg * sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream));
    }
    HIP_TRY(hipEventRecord(s->ev[4], s->stream));
    HIP_TRY(hipEventSynchronize(s->ev[1]));  // the staging may be filled again
    s->n = n;
    s->nseg = nseg;
    s->first = p->fresh;
    p->fresh = last;
    p->queued();
    return UTM_OK;
}

extern "C" int utm_deflate_pull(utm_deflate *p, const uint8_t **out, uint64_t *out_bytes)
{
    BATCH_CTX(p, "deflate");
    if (!out || !out_bytes) return fail(UTM_EINVAL, "out or out_bytes is NULL");
    *out = nullptr;
    *out_bytes = 0;
    DefSlot *s;
    TRY(p->take_oldest("pull", &s));
    HIP_TRY(hipStreamSynchronize(s->stream));
    const u64 total = s->nseg ? s->h_info[0] : 0;
    HIP_TRY(hipEventRecord(s->ev[5], s->stream));
    if (total) HIP_TRY(hipMemcpyAsync(s->h_out, s->d_out, total, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipEventRecord(s->ev[6], s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    TRY(add_elapsed(&p->ms[0], s->ev[0], s->ev[1]));
    TRY(add_elapsed(&p->ms[1], s->ev[1], s->ev[4]));
    TRY(add_elapsed(&p->ms[2], s->ev[5], s->ev[6]));
    TRY(add_elapsed(&p->ms[3], s->ev[2], s->ev[3]));
    if (s->first) p->a = 1, p->b = 0;
    for (uint32_t g = 0; g < s->nseg; ++g)
        def_adler_add(&p->a, &p->b, std::min<u64>(DEF_SEG, s->n - (u64)g * DEF_SEG), s->h_info[1 + 2 * g], s->h_info[2 + 2 * g]);
    *out = s->h_out;
    *out_bytes = total;
    return UTM_OK;
}

extern "C" int utm_deflate_adler(utm_deflate *p, uint32_t *adler)
{
    if (!p || !adler) return fail(UTM_EINVAL, "deflate or adler is NULL");
    *adler = p->b << 16 | p->a;
    return UTM_OK;
}

extern "C" int utm_deflate_timing(utm_deflate *p, double *ms)
{
    if (!p || !ms) return fail(UTM_EINVAL, "deflate or ms is NULL");
    for (int i = 0; i < 4; ++i) ms[i] = p->ms[i];
    return UTM_OK;
}

// The kernels' code run on the CPU with one lane, segment by segment: the same bytes as the device.
extern "C" int utm_deflate_host(const uint8_t *in, uint64_t n_bytes, int level, uint8_t *out, uint64_t out_cap,
                                uint64_t *out_bytes, uint32_t *adler)
{
    if (!out_bytes || !adler || (n_bytes && !in) || (out_cap && !out)) return fail(UTM_EINVAL, "in, out, out_bytes or adler is NULL");
    TRY(def_check_level(level));
    const DefLevel lv = def_level(level);
    std::vector<uint32_t> seg((DEF_SEG + DEF_PAD) / 4), so(DEF_SEG_OUT / 4), match(DEF_SEG), tok(DEF_SEG), head(DEF_HSIZE);
    std::vector<uint16_t> prev(DEF_SEG);
    std::vector<DefTables> t(1);
    uint8_t *sb = reinterpret_cast<uint8_t *>(seg.data());
    const uint64_t nseg = std::max<uint64_t>(1, (n_bytes + DEF_SEG - 1) / DEF_SEG);
    uint32_t a = 1, b = 0;
    u64 done = 0;
    for (u64 g = 0; g < nseg; ++g) {
        const uint32_t n = (uint32_t)std::min<u64>(DEF_SEG, n_bytes - g * DEF_SEG);
        std::fill(seg.begin(), seg.end(), 0u);
        if (n) memcpy(sb, in + g * DEF_SEG, n);
        def_chain(sb, n, prev.data(), head.data(), 0, 1);
        for (uint32_t q = 0; q < n; ++q) match[q] = def_match(sb, n, prev.data(), q, lv);
        uint32_t q = 0, k = 0;
        while (q < n) {
            uint32_t adv;
            tok[k++] = def_step(match[q], q + 1 < n ? match[q + 1] : 0, sb[q], lv.lazy, &adv);
            q += adv;
        }
        uint32_t sums[2];
        const uint32_t bytes = def_encode(sb, n, tok.data(), k, g == nseg - 1, reinterpret_cast<uint8_t *>(so.data()),
                                          sums, t.data(), 0, 1);
        if (bytes > out_cap - done)
            return fail(UTM_EINVAL, "out_cap %llu is too small (utm_deflate_bound(%llu) = %llu)", (unsigned long long)out_cap,
                        (unsigned long long)n_bytes, (unsigned long long)def_bound(n_bytes));
        memcpy(out + done, so.data(), bytes);
        done += bytes;
        def_adler_add(&a, &b, n, sums[0], sums[1]);
    }
    *out_bytes = done;
    *adler = b << 16 | a;
    return UTM_OK;
}
