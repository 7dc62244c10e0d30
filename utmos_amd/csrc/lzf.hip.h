// LZF chunks of an HDF5 store on the GPU: the reference's `--lowmem` store keeps its `data` dataset as h5py LZF
// chunks of whole rows (one byte per cell for bool, four for float32 GT * AF).  Decoded, a chunk is 8x / 32x larger than
// its packed rows, so the chunks are decoded and packed here and only the packed rows leave the device.
//
//   k_lzf_decode   one 64-lane workgroup per chunk: lane 0 parses up to LZF_TOKS tokens from an LDS window of the
//                  input into an LDS list, then all lanes copy them, token by token, into an 8 KiB LDS ring (LZF
//                  reaches at most 8 KiB back); the batch's bytes leave the ring as 16 B stores.  Raw chunks (filter
//                  mask bit 0) are copied, absent ones (stored size 0) read as fill (zeros).
//   k_h5_pack      one wave per decoded row: a ballot of 64 cells is 8 packbits bytes once each byte's bits are
//                  reversed (numpy order: cell 0 is the MSB of byte 0); float32 rows also give their common nonzero
//                  value (the row's AF), and a row whose nonzero values differ, or are negative or NaN, marks its chunk.
//
// The token parser (lzf_token) is __host__ __device__: utm_lzf_decode_host runs it on the CPU.  It never reads a byte
// at or past the end it is given, and a token that would write past the chunk or reach before its start is an
// LZF_E_* code: a malformed chunk ends in its status word, never in a fault.
#pragma once
#include "common.hip.h"

#define LZF_THREADS 64
#define LZF_RING 8192u   // LZF offsets reach 8,192 bytes back: the ring holds exactly that much history
#define LZF_WIN 4096u    // input window in LDS (a token is at most 33 bytes, so a window holds 64 of them)
#define LZF_TOKS 64u     // tokens parsed per batch
#define H5_PACK_THREADS 256

// chunk status word (0 = good)
#define LZF_E_INPUT 1    // a token runs past the chunk's stored bytes
#define LZF_E_OUTPUT 2   // more output than the chunk holds (or a raw chunk larger than the chunk)
#define LZF_E_SHORT 3    // less output than the chunk holds (or a raw chunk smaller than the chunk)
#define LZF_E_BACKREF 4  // a back-reference before the start of the chunk
#define H5_E_VALUES 5    // float32 data: a row's nonzero values differ, or one is negative or NaN

#define LZF_HD __host__ __device__ __forceinline__

struct LzfTok {
    uint32_t len;  // bytes of output
    uint32_t off;  // back-reference distance; 0 = a literal run
    uint32_t src;  // a literal's first byte in the input
};

// One token at in(pos), pos < n_in: a literal run of c + 1 bytes (control byte c < 32), or a back-reference of
// (c >> 5) + 2 bytes (7 -> one more length byte) at distance ((c & 31) << 8) + next + 1.  `out` = bytes written so far.
template <class IN>
LZF_HD int lzf_token(const IN &in, uint32_t pos, uint32_t n_in, uint32_t out, uint32_t n_out, LzfTok *t, uint32_t *next)
{
    const uint32_t c = in(pos);
    if (c < 32) {
        t->len = c + 1;
        t->off = 0;
        t->src = pos + 1;
        if (t->len > n_in - pos - 1) return LZF_E_INPUT;
        if (t->len > n_out - out) return LZF_E_OUTPUT;
        *next = pos + 1 + t->len;
        return 0;
    }
    uint32_t len = (c >> 5) + 2, p = pos + 1;
    if (len == 9) {
        if (p >= n_in) return LZF_E_INPUT;
        len += in(p++);
    }
    if (p >= n_in) return LZF_E_INPUT;
    const uint32_t off = ((c & 31) << 8) + in(p++) + 1;
    if (off > out) return LZF_E_BACKREF;
    if (len > n_out - out) return LZF_E_OUTPUT;
    t->len = len;
    t->off = off;
    t->src = 0;
    *next = p;
    return 0;
}

struct LzfChunk {      // one chunk of a batch (host_h5.hip.h fills the table)
    u64 off;           // first stored byte in the batch's input
    uint32_t size;     // stored bytes; 0 = the chunk is absent (fill)
    uint32_t mask;     // HDF5 filter mask: bit 0 = stored raw
    uint32_t rows;     // rows of the chunk below the dataset's end (packed)
    uint32_t row0;     // its first row among the batch's packed rows
};

struct LzfWinIn {      // reads chunk byte p from the LDS window, which holds chunk bytes [lo, lo + LZF_WIN)
    const uint8_t *w;
    int lo;
    __device__ uint32_t operator()(uint32_t p) const { return w[(int)p - lo]; }
};

__global__ __launch_bounds__(LZF_THREADS) void k_lzf_decode(const uint8_t *__restrict__ in,
                                                           const LzfChunk *__restrict__ chunks, uint32_t n_out,
                                                           u64 out_stride, uint8_t *__restrict__ out,
                                                           uint32_t *__restrict__ status)
{
    __shared__ v4u ring4[LZF_RING / 16];
    __shared__ v4u win4[LZF_WIN / 16];
    __shared__ uint32_t tok_len[LZF_TOKS], tok_arg[LZF_TOKS];
    __shared__ uint32_t ctl[3];  // tokens parsed, next input byte, error
    uint8_t *ring = reinterpret_cast<uint8_t *>(ring4);
    const uint8_t *win = reinterpret_cast<const uint8_t *>(win4);
    const unsigned lane = threadIdx.x;
    const LzfChunk ch = chunks[blockIdx.x];
    const u64 base = ch.off;
    const uint32_t n_in = ch.size;
    uint8_t *dst = out + (u64)blockIdx.x * out_stride;  // 16-byte aligned

    if (n_in == 0 || (ch.mask & 1)) {  // absent: fill; raw: copy
        if (n_in && n_in != n_out) {
            if (lane == 0) status[blockIdx.x] = n_in < n_out ? LZF_E_SHORT : LZF_E_OUTPUT;
            return;
        }
        const uint8_t *src = in + base;
        for (uint32_t i = lane * 16; i < n_out; i += LZF_THREADS * 16) {
            if (i + 16 <= n_out) {
                v4u v = {0, 0, 0, 0};
                if (n_in) {
                    uint8_t b[16];
                    for (int k = 0; k < 16; ++k) b[k] = src[i + k];
                    __builtin_memcpy(&v, b, 16);
                }
                *reinterpret_cast<v4u *>(dst + i) = v;
            } else {
                for (uint32_t k = i; k < n_out; ++k) dst[k] = n_in ? src[k] : 0;
            }
        }
        if (lane == 0) status[blockIdx.x] = 0;
        return;
    }

    uint32_t pos = 0, o = 0, err = 0;
    while (pos < n_in && !err) {
        // window: the 16-byte aligned LZF_WIN bytes of the batch input from the one holding chunk byte pos (the input
        // buffer has LZF_WIN bytes of slack behind the staging, so the loads stay inside it)
        const u64 a0 = (base + pos) & ~(u64)15;
        const int lo = (int)(a0 - base);  // chunk position of window byte 0 (at most 15 before the chunk)
        for (uint32_t i = lane; i < LZF_WIN / 16; i += LZF_THREADS)
            win4[i] = *reinterpret_cast<const v4u *>(in + a0 + 16 * i);
        __syncthreads();
        if (lane == 0) {
            const uint32_t avail = (uint32_t)min((int64_t)n_in, (int64_t)lo + LZF_WIN);
            const LzfWinIn rd{win, lo};
            uint32_t k = 0, bytes = 0, p = pos, oo = o;
            int e = 0;
            while (k < LZF_TOKS && p < avail) {
                LzfTok t;
                uint32_t nx;
                e = lzf_token(rd, p, avail, oo, n_out, &t, &nx);
                if (e) {
                    if (e == LZF_E_INPUT && avail < n_in) e = 0;  // the token continues past the window: reload
                    break;
                }
                if (bytes + t.len > LZF_RING) break;  // the ring holds one batch's output
                tok_len[k] = t.len;
                tok_arg[k] = t.off ? t.off : (0x80000000u | (uint32_t)((int)t.src - lo));
                ++k;
                bytes += t.len;
                oo += t.len;
                p = nx;
            }
            if (k == 0 && !e) e = LZF_E_INPUT;  // no progress (cannot happen with a 4 KiB window; never loop)
            ctl[0] = k;
            ctl[1] = p;
            ctl[2] = (uint32_t)e;
        }
        __syncthreads();
        const uint32_t k = ctl[0], o0 = o;
        err = ctl[2];
        for (uint32_t t = 0; t < k; ++t) {
            const uint32_t len = tok_len[t], arg = tok_arg[t];
            for (uint32_t j = lane; j < len; j += LZF_THREADS) {
                uint8_t v;
                if (arg & 0x80000000u) {
                    v = win[(arg & 0x7fffffffu) + j];
                } else {  // off < len: the last `off` bytes repeat; every lane reads history, none reads this token
                    const uint32_t q = arg >= len ? j : j % arg;
                    v = ring[(o - arg + q) & (LZF_RING - 1)];
                }
                ring[(o + j) & (LZF_RING - 1)] = v;
            }
            o += len;
            __syncthreads();
        }
        // the batch's bytes [o0, o): at most LZF_RING of them, all still in the ring
        const uint32_t head = min(o, (o0 + 15) & ~15u);
        for (uint32_t q = o0 + lane; q < head; q += LZF_THREADS) dst[q] = ring[q & (LZF_RING - 1)];
        const uint32_t tail = max(head, o & ~15u);
        for (uint32_t q = head + lane * 16; q < tail; q += LZF_THREADS * 16)
            *reinterpret_cast<v4u *>(dst + q) = ring4[(q & (LZF_RING - 1)) >> 4];
        for (uint32_t q = tail + lane; q < o; q += LZF_THREADS) dst[q] = ring[q & (LZF_RING - 1)];
        pos = ctl[1];
        __syncthreads();  // the window and the token list are read by everybody before lane 0 reuses them
    }
    if (!err && o != n_out) err = LZF_E_SHORT;
    if (lane == 0) status[blockIdx.x] = err;
}

// Decoded rows -> packbits rows (numpy order) and, for float32 cells, the row's common nonzero value.  Rows of a chunk
// whose decode failed are left alone.
__global__ __launch_bounds__(H5_PACK_THREADS) void k_h5_pack(const uint8_t *__restrict__ dec, u64 dec_stride,
                                                            const LzfChunk *__restrict__ chunks, uint32_t n_cols,
                                                            uint32_t itemsize, uint8_t *__restrict__ rows,
                                                            float *__restrict__ af, uint32_t *__restrict__ status)
{
    const unsigned lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const LzfChunk ch = chunks[blockIdx.x];
    if (status[blockIdx.x]) return;
    const uint32_t row_bytes = (n_cols + 7) >> 3;
    const uint8_t *cells = dec + (u64)blockIdx.x * dec_stride;
    bool bad_chunk = false;
    for (uint32_t r = wave; r < ch.rows; r += H5_PACK_THREADS / 64) {
        uint8_t *dst = rows + (u64)(ch.row0 + r) * row_bytes;
        uint32_t val = 0;   // float bits of this lane's nonzero cells (0: none seen)
        bool bad = false;
        for (uint32_t g = 0; g < n_cols; g += 64) {
            const uint32_t col = g + lane;
            bool set = false;
            if (col < n_cols) {
                const u64 cell = (u64)r * n_cols + col;
                if (itemsize == 1) {
                    set = cells[cell] != 0;
                } else {
                    const float f = reinterpret_cast<const float *>(cells)[cell];
                    set = f != 0.0f;
                    if (set) {
                        const uint32_t bits = __float_as_uint(f);
                        bad |= !(f > 0.0f) || (val && bits != val);  // negative or NaN, or a second value
                        val = bits;
                    }
                }
            }
            const u64 m = __ballot(set);
            if (lane < 8 && g / 8 + lane < row_bytes)
                dst[g / 8 + lane] = (uint8_t)(__builtin_bitreverse32((uint32_t)(m >> (8 * lane)) & 0xffu) >> 24);
        }
        if (itemsize == 4) {
            const u64 holders = __ballot(val != 0);
            const uint32_t common = holders ? (uint32_t)__shfl((int)val, __ffsll((long long)holders) - 1) : 0u;
            bad |= val && val != common;
            if (__ballot(bad)) bad_chunk = true;
            if (lane == 0) af[ch.row0 + r] = __uint_as_float(common);
        }
    }
    if (bad_chunk && lane == 0) status[blockIdx.x] = H5_E_VALUES;
}
