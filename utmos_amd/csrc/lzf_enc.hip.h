// LZF encoding of HDF5 chunks on the GPU: the writer side of lzf.hip.h.  The reference's `--lowmem` store keeps its
// `data` dataset as h5py LZF chunks of whole rows; the packed rows the loader already holds are expanded to the
// chunk's cells here and compressed with the exact parse h5py's filter runs (liblzf's lzf_compress as h5py builds it),
// so the stored bytes equal the reference's byte for byte.
//
//   k_h5_cells     packbits rows -> cells: one byte per cell (h5py's bool enum) or float32 GT * AF; the rows past the
//                  batch's last one are zero (a partial last chunk is stored full size)
//   k_lzf_encode   one wave per chunk: the parse is serial, every lane runs it in step and the lanes share the work
//                  that exactness allows (the 64-byte steps of a match's extension, the table reset); lane 0 stores
//   k_deflate_scan / k_h5w_gather   the stored chunks (compressed, or raw when LZF does not fit) packed back to back
//
// The parse (lzf_encode) is __host__ __device__ and takes its hash table, input and match extension as policies:
// utm_lzf_encode_host runs it on the CPU with liblzf's full 2^17-slot table, the device with LzfWaveTable.
//
// liblzf's table holds, per 17-bit slot, the last position written into it; a position is a match candidate only if
// it lies at most 8,192 bytes back.  The slot's last write is either inside that window, or no write into the slot is,
// so "the most recent in-window position with this slot" answers the same.  LzfWaveTable keeps exactly the window's
// live positions in LDS (48 KiB): head[slot & 4095] is the bucket's newest position, ring[q & 8191] holds position q's
// 17-bit slot and the distance back to the bucket's previous position.  A lookup walks the bucket's chain, newest
// first, until a position's slot matches or the chain leaves the window.  A position in the window was written within
// the last 8,192 steps, so its ring entry is still its own.
#pragma once
#include "common.hip.h"

#define LZFE_THREADS 64
#define LZFE_HLOG 17
#define LZFE_MAX_LIT 32u
#define LZFE_MAX_OFF 8192u
#define LZFE_MAX_REF 264u          // (1 << 8) + (1 << 3)
#define LZFE_BUCKETS 4096u         // LzfWaveTable chain heads
#define LZFE_RING 8192u            // LzfWaveTable: one entry per position of the window
#define LZFE_NONE 0xffffffffu
#define H5W_CELLS_THREADS 256
#define H5W_GATHER_THREADS 256

LZF_HD uint32_t lzfe_slot(uint32_t h) { return ((h >> (24 - LZFE_HLOG)) - h) & ((1u << LZFE_HLOG) - 1); }

// One chunk in(0 .. n) -> out[0, size); returns size, or 0 when the output does not fit in out_len bytes (liblzf's own
// checks; the chunk is then stored raw).  Every store of a byte goes through put(at, v).
//   TAB:  uint32_t swap(slot, p)  -> the slot's last position (0 = none), p written in its place
//         void     set(slot, p)
//   EXT:  uint32_t ext(r, p, maxlen) -> the first k >= 3 with k == maxlen or in(r + k) != in(p + k)
template <class IN, class PUT, class TAB, class EXT>
LZF_HD uint32_t lzf_encode(const IN &in, uint32_t n, uint32_t out_len, const PUT &put, TAB &tab, const EXT &ext)
{
    if (n == 0 || out_len == 0) return 0;
    uint32_t op = 1, lit = 0, p = 0;
    uint32_t h = n >= 2 ? (in(0) << 8 | in(1)) : 0;
    while (p + 2 < n) {
        h = (h << 8) | in(p + 2);
        const uint32_t slot = lzfe_slot(h);
        const uint32_t r = tab.swap(slot, p);
        if (r > 0 && p - r - 1 < LZFE_MAX_OFF && p + 4 < n && in(r) == in(p) && in(r + 1) == in(p + 1) &&
            in(r + 2) == in(p + 2)) {
            const uint32_t off = p - r - 1;
            const uint32_t maxlen = n - p - 2 < LZFE_MAX_REF ? n - p - 2 : LZFE_MAX_REF;
            const uint32_t len = ext(r, p, maxlen);
            if (op + 4 >= out_len && op - (lit == 0) + 4 >= out_len) return 0;
            put(op - lit - 1, (uint8_t)(lit - 1));  // stop the literal run (a run of 0 is taken back below)
            op -= lit == 0;
            const uint32_t code = len - 2;
            if (code < 7) {
                put(op++, (uint8_t)((off >> 8) + (code << 5)));
            } else {
                put(op++, (uint8_t)((off >> 8) + (7u << 5)));
                put(op++, (uint8_t)(code - 7));
            }
            put(op, (uint8_t)off);
            op += 2;  // the offset byte and the next run's control byte
            lit = 0;
            p += len;
            if (p + 2 >= n) break;
            const uint32_t q = p - 1;  // ULTRA_FAST: only the match's last position goes into the table
            h = (in(q) << 16) | (in(q + 1) << 8) | in(q + 2);
            tab.set(lzfe_slot(h), q);
        } else {
            if (op >= out_len) return 0;
            put(op++, (uint8_t)in(p++));
            if (++lit == LZFE_MAX_LIT) {
                put(op - lit - 1, (uint8_t)(lit - 1));
                lit = 0;
                ++op;
            }
        }
    }
    if (op + 3 > out_len) return 0;
    while (p < n) {
        put(op++, (uint8_t)in(p++));
        if (++lit == LZFE_MAX_LIT) {
            put(op - lit - 1, (uint8_t)(lit - 1));
            lit = 0;
            ++op;
        }
    }
    put(op - lit - 1, (uint8_t)(lit - 1));
    op -= lit == 0;
    return op;
}

// ------------------------------------------------------------------------------------------------ device
struct LzfWaveTable {
    uint32_t *head;  // [LZFE_BUCKETS] newest position of the bucket, LZFE_NONE = none
    uint32_t *ring;  // [LZFE_RING] position q: slot | (distance to the bucket's previous position, 0 = none) << 17
    __device__ uint32_t find(uint32_t slot, uint32_t p) const
    {
        uint32_t x = head[slot & (LZFE_BUCKETS - 1)];
        while (x != LZFE_NONE && x + LZFE_MAX_OFF >= p) {
            const uint32_t e = ring[x & (LZFE_RING - 1)];
            if ((e & 0x1ffffu) == slot) return x;
            const uint32_t d = e >> 17;
            if (d == 0 || d > x) break;
            x -= d;
        }
        return 0;  // none in the window (liblzf's table may hold an older position: too far back either way)
    }
    __device__ void set(uint32_t slot, uint32_t p)
    {
        uint32_t *hd = &head[slot & (LZFE_BUCKETS - 1)];
        const uint32_t prev = *hd;
        const uint32_t d = prev != LZFE_NONE && p - prev <= LZFE_MAX_OFF ? p - prev : 0;
        ring[p & (LZFE_RING - 1)] = slot | (d << 17);
        *hd = p;
    }
    __device__ uint32_t swap(uint32_t slot, uint32_t p)
    {
        const uint32_t r = find(slot, p);
        set(slot, p);
        return r;
    }
};

struct LzfGlobalIn {
    const uint8_t *p;
    __device__ uint32_t operator()(uint32_t i) const { return p[i]; }
};

struct LzfWavePut {  // lane 0 stores; the other lanes hold the same bytes
    uint8_t *out;
    unsigned lane;
    __device__ void operator()(uint32_t at, uint8_t v) const
    {
        if (lane == 0) out[at] = v;
    }
};

struct LzfWaveExt {  // 64 positions of the match per step, the first unequal one by ballot
    const uint8_t *in;
    unsigned lane;
    __device__ uint32_t operator()(uint32_t r, uint32_t p, uint32_t maxlen) const
    {
        uint32_t len = 3;
        while (len < maxlen) {
            const uint32_t k = len + lane;
            const bool stop = k >= maxlen || in[r + k] != in[p + k];
            const u64 m = __ballot(stop);
            if (m) return len + (uint32_t)(__ffsll((long long)m) - 1);
            len += LZFE_THREADS;
        }
        return maxlen;
    }
};

// grid-stride over the batch's cells: cell (row, col) of chunk-major storage is row r = chunk * chunk_rows + row
__global__ __launch_bounds__(H5W_CELLS_THREADS) void k_h5_cells(const uint8_t *__restrict__ rows,
                                                               const float *__restrict__ af, u64 n_rows,
                                                               u64 total_rows, uint32_t n_cols, uint32_t itemsize,
                                                               uint8_t *__restrict__ cells)
{
    const uint32_t row_bytes = (n_cols + 7) >> 3;
    const u64 n_cells = total_rows * n_cols;
    for (u64 i = (u64)blockIdx.x * H5W_CELLS_THREADS + threadIdx.x; i < n_cells; i += (u64)gridDim.x * H5W_CELLS_THREADS) {
        const u64 r = i / n_cols;
        const uint32_t c = (uint32_t)(i - r * n_cols);
        const uint32_t gt = r < n_rows ? (rows[r * row_bytes + (c >> 3)] >> (7 - (c & 7))) & 1u : 0u;
        if (itemsize == 1)
            cells[i] = (uint8_t)gt;
        else  // float32(GT * AF) as numpy computes it: 0 * AF keeps AF's sign and NaN
            reinterpret_cast<float *>(cells)[i] = r < n_rows ? (float)gt * af[r] : 0.0f;
    }
}

// one wave per chunk: cells[chunk * chunk_bytes, +chunk_bytes) -> enc (same stride); stored[chunk] = the compressed
// size, or chunk_bytes with masks[chunk] = 1 when LZF does not fit (h5py's filter gives it chunk_bytes of room)
__global__ __launch_bounds__(LZFE_THREADS) void k_lzf_encode(const uint8_t *__restrict__ cells, uint32_t chunk_bytes,
                                                            uint8_t *__restrict__ enc, uint32_t *__restrict__ stored,
                                                            uint32_t *__restrict__ masks)
{
    __shared__ uint32_t head[LZFE_BUCKETS];
    __shared__ uint32_t ring[LZFE_RING];
    const unsigned lane = threadIdx.x;
    for (uint32_t i = lane; i < LZFE_BUCKETS; i += LZFE_THREADS) head[i] = LZFE_NONE;
    __syncthreads();
    const u64 base = (u64)blockIdx.x * chunk_bytes;
    LzfWaveTable tab{head, ring};
    const uint32_t size = lzf_encode(LzfGlobalIn{cells + base}, chunk_bytes, chunk_bytes, LzfWavePut{enc + base, lane},
                                     tab, LzfWaveExt{cells + base, lane});
    if (lane == 0) {
        stored[blockIdx.x] = size ? size : chunk_bytes;
        masks[blockIdx.x] = size ? 0u : 1u;
    }
}

// grid: (chunks): the chunk's stored bytes (compressed from enc, raw from cells) to out + offs[chunk]
__global__ __launch_bounds__(H5W_GATHER_THREADS) void k_h5w_gather(const uint8_t *__restrict__ cells,
                                                                  const uint8_t *__restrict__ enc, uint32_t chunk_bytes,
                                                                  const uint32_t *__restrict__ stored,
                                                                  const uint32_t *__restrict__ masks,
                                                                  const uint32_t *__restrict__ offs,
                                                                  uint8_t *__restrict__ out)
{
    const uint32_t c = blockIdx.x, n = stored[c];
    const uint8_t *src = ((masks[c] & 1) ? cells : enc) + (u64)c * chunk_bytes;
    uint8_t *dst = out + offs[c];
    for (uint32_t i = threadIdx.x; i < n; i += H5W_GATHER_THREADS) dst[i] = src[i];
}
