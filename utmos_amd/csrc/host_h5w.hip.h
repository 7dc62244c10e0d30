// HDF5 chunk writer context (utm_h5w_*): host side of lzf_enc.hip.h.  Batches of packbits rows become the stored
// chunks of the reference's `data` dataset (cells built, LZF-encoded, raw where LZF does not fit, packed back to back)
// on the device; the caller gets the batch's stored bytes, each chunk's stored size and its HDF5 filter mask.
//
// One pinned staging buffer and two slots (host_batch.hip.h): utm_h5w_encode returns once its rows have reached the
// device and the kernels are queued, so the caller fills the staging with the next batch while the GPU encodes;
// utm_h5w_fetch collects the oldest batch.
#pragma once

struct H5wSlot : BatchSlot<6> {  // events around: H2D (0-1), cells (1-2), encode + scan + gather (2-3), D2H (4-5)
    Scratch<uint8_t> d_rows, d_cells, d_enc, d_out;
    Scratch<float> d_af;
    Scratch<uint32_t> d_stored, d_masks, d_offs;
    Pinned<uint8_t> h_out;
    Pinned<float> h_af;
    Pinned<uint32_t> h_stored, h_masks, h_offs;
    uint32_t n_chunks = 0;
};

struct utm_h5w : SlotPair<H5wSlot> {
    int device = 0;
    uint32_t chunk_rows = 0, n_cols = 0, itemsize = 0, max_chunks = 0;
    u64 chunk_bytes = 0, row_bytes = 0, stage_cap = 0;
    Pinned<uint8_t> h_stage;
    double ms[4] = {0, 0, 0, 0};  // H2D, cells, encode, D2H
    ~utm_h5w() { idle(device); }
};

extern "C" int utm_h5w_create(int device, uint32_t chunk_rows, uint32_t n_cols, uint32_t itemsize, uint32_t max_chunks,
                              utm_h5w **out)
{
    if (!out) return fail(UTM_EINVAL, "out is NULL");
    *out = nullptr;
    if (max_chunks == 0 || max_chunks > UTM_H5_MAX_CHUNKS) return fail(UTM_EINVAL, "max_chunks %u not in [1, 65536]", max_chunks);
    if (itemsize != 1 && itemsize != 4) return fail(UTM_EINVAL, "itemsize %u is neither 1 nor 4", itemsize);
    if (chunk_rows == 0 || n_cols == 0) return fail(UTM_EINVAL, "a chunk of %u x %u cells", chunk_rows, n_cols);
    const u64 chunk_bytes = (u64)chunk_rows * n_cols * itemsize;
    if (chunk_bytes > UTM_H5_MAX_CHUNK_BYTES)
        return fail(UTM_EINVAL, "a chunk of %llu bytes (at most 2^31 - 2^16)", (unsigned long long)chunk_bytes);
    if (chunk_bytes * max_chunks > UTM_H5W_MAX_BATCH_BYTES)
        return fail(UTM_EINVAL, "%u chunks of %llu bytes: more than 2^32 - 2^16 bytes per batch", max_chunks,
                    (unsigned long long)chunk_bytes);
    TRY(open_device(device));
    std::unique_ptr<utm_h5w> p(new utm_h5w());
    p->device = device;
    p->chunk_rows = chunk_rows;
    p->n_cols = n_cols;
    p->itemsize = itemsize;
    p->max_chunks = max_chunks;
    p->chunk_bytes = chunk_bytes;
    p->row_bytes = (n_cols + 7) / 8;
    const u64 nc = max_chunks, rows = nc * chunk_rows;
    p->stage_cap = rows * p->row_bytes;
    TRY(p->h_stage.reserve(p->stage_cap));
    for (H5wSlot &s : p->slot) {
        TRY(s.open());
        TRY(s.d_rows.reserve(p->stage_cap));
        TRY(s.d_af.reserve(rows));
        TRY(s.d_cells.reserve(nc * chunk_bytes));
        TRY(s.d_enc.reserve(nc * chunk_bytes));
        TRY(s.d_out.reserve(nc * chunk_bytes));
        TRY(s.d_stored.reserve(nc));
        TRY(s.d_masks.reserve(nc));
        TRY(s.d_offs.reserve(nc + 1));
        TRY(s.h_out.reserve(nc * chunk_bytes));
        TRY(s.h_af.reserve(rows));
        TRY(s.h_stored.reserve(nc));
        TRY(s.h_masks.reserve(nc));
        TRY(s.h_offs.reserve(nc + 1));
    }
    *out = p.release();
    return UTM_OK;
}

extern "C" int utm_h5w_destroy(utm_h5w *p)
{
    delete p;
    return UTM_OK;
}

extern "C" int utm_h5w_staging(utm_h5w *p, uint8_t **buf, uint64_t *cap)
{
    if (!p || !buf || !cap) return fail(UTM_EINVAL, "h5w, buf or cap is NULL");
    *buf = p->h_stage;
    *cap = p->stage_cap;
    return UTM_OK;
}

extern "C" int utm_h5w_encode(utm_h5w *p, const uint8_t *rows, const float *af, uint64_t n_rows)
{
    BATCH_CTX(p, "h5w");
    const u64 cap_rows = (u64)p->max_chunks * p->chunk_rows;
    if (n_rows == 0 || n_rows > cap_rows)
        return fail(UTM_EINVAL, "n_rows %llu not in [1, %llu]", (unsigned long long)n_rows, (unsigned long long)cap_rows);
    if (!rows) return fail(UTM_EINVAL, "rows is NULL");
    if (p->itemsize == 4 && !af) return fail(UTM_EINVAL, "af is NULL (a float32 store)");
    H5wSlot *s;
    TRY(p->free_slot("utm_h5w_fetch", &s));
    const uint32_t n_chunks = (uint32_t)((n_rows + p->chunk_rows - 1) / p->chunk_rows);
    const u64 row_bytes = n_rows * p->row_bytes, total_rows = (u64)n_chunks * p->chunk_rows;
    if (rows != p->h_stage) memcpy(p->h_stage, rows, row_bytes);
    if (p->itemsize == 4) memcpy(s->h_af, af, n_rows * sizeof(float));
    HIP_TRY(hipEventRecord(s->ev[0], s->stream));
    HIP_TRY(hipMemcpyAsync(s->d_rows, p->h_stage, row_bytes, hipMemcpyHostToDevice, s->stream));
    if (p->itemsize == 4) HIP_TRY(hipMemcpyAsync(s->d_af, s->h_af, n_rows * sizeof(float), hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipEventRecord(s->ev[1], s->stream));
    const u64 n_cells = total_rows * p->n_cols;
    const u64 blocks = std::min<u64>((n_cells + H5W_CELLS_THREADS - 1) / H5W_CELLS_THREADS, 8192);
    k_h5_cells<<<(unsigned)blocks, H5W_CELLS_THREADS, 0, s->stream>>>(s->d_rows, s->d_af, n_rows, total_rows, p->n_cols,
                                                                      p->itemsize, s->d_cells);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(s->ev[2], s->stream));
    k_lzf_encode<<<n_chunks, LZFE_THREADS, 0, s->stream>>>(s->d_cells, (uint32_t)p->chunk_bytes, s->d_enc, s->d_stored,
                                                           s->d_masks);
    HIP_TRY(hipGetLastError());
    k_deflate_scan<<<1, DEF_THREADS, 0, s->stream>>>(s->d_stored, n_chunks, s->d_offs);
    HIP_TRY(hipGetLastError());
    k_h5w_gather<<<n_chunks, H5W_GATHER_THREADS, 0, s->stream>>>(s->d_cells, s->d_enc, (uint32_t)p->chunk_bytes,
                                                                 s->d_stored, s->d_masks, s->d_offs, s->d_out);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(s->ev[3], s->stream));
    HIP_TRY(hipMemcpyAsync(s->h_stored, s->d_stored, n_chunks * sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipMemcpyAsync(s->h_masks, s->d_masks, n_chunks * sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipMemcpyAsync(s->h_offs, s->d_offs, (n_chunks + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipEventSynchronize(s->ev[1]));  // the staging may be filled again
    s->n_chunks = n_chunks;
    p->queued();
    return UTM_OK;
}

extern "C" int utm_h5w_fetch(utm_h5w *p, const uint8_t **out, uint64_t *out_bytes, uint32_t *sizes, uint32_t *masks,
                             uint32_t *n_chunks)
{
    BATCH_CTX(p, "h5w");
    if (!out || !out_bytes || !sizes || !masks || !n_chunks)
        return fail(UTM_EINVAL, "out, out_bytes, sizes, masks or n_chunks is NULL");
    H5wSlot *s;
    TRY(p->take_oldest("fetch", &s));
    HIP_TRY(hipStreamSynchronize(s->stream));  // the sizes are in: the stored bytes follow in one copy
    const u64 total = s->h_offs[s->n_chunks];
    HIP_TRY(hipEventRecord(s->ev[4], s->stream));
    if (total) HIP_TRY(hipMemcpyAsync(s->h_out, s->d_out, total, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipEventRecord(s->ev[5], s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    for (int i = 0; i < 3; ++i) TRY(add_elapsed(&p->ms[i], s->ev[i], s->ev[i + 1]));
    TRY(add_elapsed(&p->ms[3], s->ev[4], s->ev[5]));
    memcpy(sizes, s->h_stored, s->n_chunks * sizeof(uint32_t));
    memcpy(masks, s->h_masks, s->n_chunks * sizeof(uint32_t));
    *out = s->h_out;
    *out_bytes = total;
    *n_chunks = s->n_chunks;
    return UTM_OK;
}

extern "C" int utm_h5w_timing(utm_h5w *p, double *ms)
{
    if (!p || !ms) return fail(UTM_EINVAL, "h5w or ms is NULL");
    for (int i = 0; i < 4; ++i) ms[i] = p->ms[i];
    return UTM_OK;
}

// The device's LZF encoder run on the CPU, with liblzf's full table: one chunk in[0, n_in) -> out, at most out_cap
// bytes; *out_bytes = 0 when they do not fit (h5py then stores the chunk raw).
struct LzfHostTable {
    std::vector<uint32_t> t = std::vector<uint32_t>(1u << LZFE_HLOG, 0u);
    uint32_t swap(uint32_t slot, uint32_t p)
    {
        const uint32_t r = t[slot];
        t[slot] = p;
        return r;
    }
    void set(uint32_t slot, uint32_t p) { t[slot] = p; }
};

extern "C" int utm_lzf_encode_host(const uint8_t *in, uint64_t n_in, uint8_t *out, uint64_t out_cap, uint64_t *out_bytes)
{
    if (!out_bytes || (n_in && !in) || (out_cap && !out)) return fail(UTM_EINVAL, "in, out or out_bytes is NULL");
    if (n_in > UINT32_MAX - 64) return fail(UTM_EINVAL, "a chunk of 2^32 - 64 bytes or more");
    const uint32_t cap = (uint32_t)std::min<uint64_t>(out_cap, UINT32_MAX);
    LzfHostTable tab;
    const LzfHostIn rd{in};
    const auto put = [out](uint32_t at, uint8_t v) { out[at] = v; };
    const auto ext = [in](uint32_t r, uint32_t p, uint32_t maxlen) {
        uint32_t len = 3;
        while (len < maxlen && in[r + len] == in[p + len]) ++len;
        return len;
    };
    *out_bytes = lzf_encode(rd, (uint32_t)n_in, cap, put, tab, ext);
    return UTM_OK;
}
