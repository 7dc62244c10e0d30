// HDF5 chunk context (utm_h5_*): host side of lzf.hip.h.  Batches of one dataset's stored chunks (whole rows, every
// column) are decoded and packed on the device; the caller gets packbits rows, float32 AF per row and a status word
// per chunk.
//
// One pinned staging buffer and two slots (host_batch.hip.h), each with its own device buffers and pinned results:
// utm_h5_decode returns once its batch has reached the device and the kernels are queued, so the caller reads the next
// batch from the file into the staging while the GPU decodes; utm_h5_fetch collects the oldest batch.
#pragma once

struct H5Slot : BatchSlot<5> {  // events around: H2D (0-1), decode (1-2), pack (2-3), D2H (3-4)
    Scratch<uint8_t> d_in, d_dec, d_rows;
    Pinned<uint8_t> h_rows;
    Scratch<float> d_af;
    Pinned<float> h_af;
    Scratch<uint32_t> d_status;
    Pinned<uint32_t> h_status;
    Scratch<LzfChunk> d_chunks;
    Pinned<LzfChunk> h_chunks;
    uint32_t n_chunks = 0;
    u64 n_rows = 0;
};

struct utm_h5 : SlotPair<H5Slot> {
    int device = 0;
    u64 stage_cap = 0;
    uint32_t max_chunks = 0, chunk_rows = 0, n_cols = 0, itemsize = 0;
    u64 chunk_bytes = 0, dec_stride = 0, row_bytes = 0;
    Pinned<uint8_t> h_stage;
    double ms[4] = {0, 0, 0, 0};  // H2D, decode, pack, D2H
    ~utm_h5() { idle(device); }
};

extern "C" int utm_h5_create(int device, uint64_t stage_bytes, uint32_t max_chunks, uint32_t chunk_rows,
                             uint32_t n_cols, uint32_t itemsize, utm_h5 **out)
{
    if (!out) return fail(UTM_EINVAL, "out is NULL");
    *out = nullptr;
    if (stage_bytes == 0 || stage_bytes > UTM_H5_MAX_STAGE)
        return fail(UTM_EINVAL, "stage_bytes %llu not in [1, 2^31)", (unsigned long long)stage_bytes);
    if (max_chunks == 0 || max_chunks > UTM_H5_MAX_CHUNKS) return fail(UTM_EINVAL, "max_chunks %u not in [1, 65536]", max_chunks);
    if (itemsize != 1 && itemsize != 4) return fail(UTM_EINVAL, "itemsize %u is neither 1 nor 4", itemsize);
    if (chunk_rows == 0 || n_cols == 0) return fail(UTM_EINVAL, "a chunk of %u x %u cells", chunk_rows, n_cols);
    const u64 chunk_bytes = (u64)chunk_rows * n_cols * itemsize;
    if (chunk_bytes > UTM_H5_MAX_CHUNK_BYTES)
        return fail(UTM_EINVAL, "a chunk of %llu bytes (at most 2^31 - 2^16)", (unsigned long long)chunk_bytes);
    TRY(open_device(device));
    std::unique_ptr<utm_h5> p(new utm_h5());
    p->device = device;
    p->stage_cap = stage_bytes;
    p->max_chunks = max_chunks;
    p->chunk_rows = chunk_rows;
    p->n_cols = n_cols;
    p->itemsize = itemsize;
    p->chunk_bytes = chunk_bytes;
    p->dec_stride = (chunk_bytes + 15) & ~(u64)15;
    p->row_bytes = (n_cols + 7) / 8;
    const u64 nc = max_chunks, rows = nc * chunk_rows;
    TRY(p->h_stage.reserve(stage_bytes));
    for (H5Slot &s : p->slot) {
        TRY(s.open());
        TRY(s.d_in.reserve(stage_bytes + LZF_WIN));  // the decoder's window may read past the batch
        TRY(s.d_dec.reserve(nc * p->dec_stride));
        TRY(s.d_rows.reserve(rows * p->row_bytes));
        TRY(s.d_af.reserve(rows));
        TRY(s.d_status.reserve(nc));
        TRY(s.d_chunks.reserve(nc));
        TRY(s.h_rows.reserve(rows * p->row_bytes));
        TRY(s.h_af.reserve(rows));
        TRY(s.h_status.reserve(nc));
        TRY(s.h_chunks.reserve(nc));
    }
    *out = p.release();
    return UTM_OK;
}

extern "C" int utm_h5_destroy(utm_h5 *p)
{
    delete p;
    return UTM_OK;
}

extern "C" int utm_h5_staging(utm_h5 *p, uint8_t **buf, uint64_t *cap)
{
    if (!p || !buf || !cap) return fail(UTM_EINVAL, "h5, buf or cap is NULL");
    *buf = p->h_stage;
    *cap = p->stage_cap;
    return UTM_OK;
}

extern "C" int utm_h5_decode(utm_h5 *p, const uint8_t *in, uint64_t n_bytes, const uint64_t *offsets,
                             const uint64_t *sizes, const uint32_t *masks, const uint32_t *rows, uint32_t n_chunks)
{
    BATCH_CTX(p, "h5");
    if (n_chunks == 0 || n_chunks > p->max_chunks) return fail(UTM_EINVAL, "n_chunks %u not in [1, %u]", n_chunks, p->max_chunks);
    if (!offsets || !sizes || !masks || !rows) return fail(UTM_EINVAL, "offsets, sizes, masks or rows is NULL");
    if (n_bytes && !in) return fail(UTM_EINVAL, "in is NULL");
    if (n_bytes > p->stage_cap)
        return fail(UTM_EINVAL, "a batch of %llu bytes (the context takes %llu)", (unsigned long long)n_bytes, (unsigned long long)p->stage_cap);
    H5Slot *s;
    TRY(p->free_slot("utm_h5_fetch", &s));
    u64 total = 0;
    for (uint32_t i = 0; i < n_chunks; ++i) {
        if (offsets[i] > n_bytes || sizes[i] > n_bytes - offsets[i])
            return fail(UTM_EINVAL, "chunk %u: bytes [%llu, +%llu) outside the batch of %llu", i, (unsigned long long)offsets[i],
                        (unsigned long long)sizes[i], (unsigned long long)n_bytes);
        if (rows[i] > p->chunk_rows) return fail(UTM_EINVAL, "chunk %u: %u rows of a %u-row chunk", i, rows[i], p->chunk_rows);
        s->h_chunks[i] = LzfChunk{offsets[i], (uint32_t)sizes[i], masks[i], rows[i], (uint32_t)total};
        total += rows[i];
    }
    if (n_bytes && in != p->h_stage) memcpy(p->h_stage, in, n_bytes);
    HIP_TRY(hipEventRecord(s->ev[0], s->stream));
    if (n_bytes) HIP_TRY(hipMemcpyAsync(s->d_in, p->h_stage, n_bytes, hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipMemcpyAsync(s->d_chunks, s->h_chunks, n_chunks * sizeof(LzfChunk), hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipEventRecord(s->ev[1], s->stream));
    k_lzf_decode<<<n_chunks, LZF_THREADS, 0, s->stream>>>(s->d_in, s->d_chunks, (uint32_t)p->chunk_bytes, p->dec_stride,
                                                          s->d_dec, s->d_status);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(s->ev[2], s->stream));
    k_h5_pack<<<n_chunks, H5_PACK_THREADS, 0, s->stream>>>(s->d_dec, p->dec_stride, s->d_chunks, p->n_cols, p->itemsize,
                                                           s->d_rows, s->d_af, s->d_status);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(s->ev[3], s->stream));
    if (total) HIP_TRY(hipMemcpyAsync(s->h_rows, s->d_rows, total * p->row_bytes, hipMemcpyDeviceToHost, s->stream));
    if (total && p->itemsize == 4) HIP_TRY(hipMemcpyAsync(s->h_af, s->d_af, total * sizeof(float), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipMemcpyAsync(s->h_status, s->d_status, n_chunks * sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipEventRecord(s->ev[4], s->stream));
    HIP_TRY(hipEventSynchronize(s->ev[1]));  // the staging may be filled again
    s->n_chunks = n_chunks;
    s->n_rows = total;
    p->queued();
    return UTM_OK;
}

extern "C" int utm_h5_fetch(utm_h5 *p, uint8_t *rows, float *af, uint32_t *status)
{
    BATCH_CTX(p, "h5");
    const H5Slot *o = p->peek_oldest();
    if (o && (!status || (o->n_rows && !rows) || (o->n_rows && p->itemsize == 4 && !af)))
        return fail(UTM_EINVAL, "status, rows or af is NULL");
    H5Slot *s;
    TRY(p->take_oldest("fetch", &s));
    HIP_TRY(hipStreamSynchronize(s->stream));
    for (int i = 0; i < 4; ++i) TRY(add_elapsed(&p->ms[i], s->ev[i], s->ev[i + 1]));
    memcpy(status, s->h_status, s->n_chunks * sizeof(uint32_t));
    if (s->n_rows) memcpy(rows, s->h_rows, s->n_rows * p->row_bytes);
    if (s->n_rows && p->itemsize == 4) memcpy(af, s->h_af, s->n_rows * sizeof(float));
    return UTM_OK;
}

extern "C" int utm_h5_timing(utm_h5 *p, double *ms)
{
    if (!p || !ms) return fail(UTM_EINVAL, "h5 or ms is NULL");
    for (int i = 0; i < 4; ++i) ms[i] = p->ms[i];
    return UTM_OK;
}

// The device's LZF token parser run on the CPU: one chunk in[0, n_in) -> out[0, n_out).
struct LzfHostIn {
    const uint8_t *p;
    uint32_t operator()(uint32_t i) const { return p[i]; }
};

extern "C" int utm_lzf_decode_host(const uint8_t *in, uint64_t n_in, uint8_t *out, uint64_t n_out, uint32_t *status)
{
    if (!status || (n_in && !in) || (n_out && !out)) return fail(UTM_EINVAL, "in, out or status is NULL");
    if (n_in > UINT32_MAX || n_out > UINT32_MAX) return fail(UTM_EINVAL, "a chunk of 2^32 bytes or more");
    const LzfHostIn rd{in};
    uint32_t pos = 0, o = 0;
    int e = 0;
    while (pos < n_in && !e) {
        LzfTok t;
        uint32_t nx;
        e = lzf_token(rd, pos, (uint32_t)n_in, o, (uint32_t)n_out, &t, &nx);
        if (e) break;
        if (t.off == 0) {
            memcpy(out + o, in + t.src, t.len);
        } else {
            for (uint32_t j = 0; j < t.len; ++j) out[o + j] = out[o - t.off + j];
        }
        o += t.len;
        pos = nx;
    }
    if (!e && o != n_out) e = LZF_E_SHORT;
    *status = (uint32_t)e;
    return UTM_OK;
}
