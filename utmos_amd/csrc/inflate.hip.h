// BGZF inflation on the GPU: every BGZF member (a gzip member of at most 64 KiB of text, RFC 1952 around RFC 1951 raw
// DEFLATE) is decoded by one 64-lane workgroup into LDS, checked (CRC32, ISIZE) and written to its place in the text.
//
//   k_bgzf_inflate   one workgroup per member: the gzip header, stored / fixed / dynamic blocks decoded by a
//                    wave-uniform loop (Huffman tables in LDS; literals by lane 0, match copies by all lanes from the
//                    member in LDS), CRC32 per lane chunk combined with a shift table, then coalesced 16 B stores
//   k_bgzf_finish    the last batch of a file: a newline after a final record that has none
//   k_bgzf_last_nl   1 + the offset of the last '\n' of the batch (the carry into the next batch starts there)
//
// The decoder core (inf_member) is __host__ __device__: with lane 0 of 1 it is the CPU build that
// utm_bgzf_inflate_host exports for tests.  It never reads outside [in, in + in_size) nor writes outside out[0, isize)
// and its tables, whatever the input; a malformed member ends with an INF_E_* code.
#pragma once
#include "common.hip.h"

#define INF_THREADS 64
#define INF_OUT_MAX 65536u  // BGZF: at most 64 KiB of text per member
#define INF_FAST_BITS 10    // first-level Huffman lookup; longer codes take the canonical walk
#define INF_WIN 64          // input window in LDS: one byte per lane per refill

// member status word: bits 0-7 an INF_E_* code (0 = good), bits 8.. the bytes decoded
#define INF_E_HEADER 1      // not a gzip deflate member, or its header runs past the member
#define INF_E_BTYPE 2       // block type 3
#define INF_E_STORED 3      // stored block with LEN != ~NLEN
#define INF_E_OVERSUB 4     // over-subscribed code lengths
#define INF_E_INCOMPLETE 5  // incomplete code lengths
#define INF_E_CODE 6        // a bit pattern no code has, or a length / distance symbol that does not exist
#define INF_E_LENS 7        // bad dynamic header: too many symbols, repeat with nothing before, repeat past the end, no end-of-block code
#define INF_E_DIST 8        // a distance behind the start of the member
#define INF_E_OUTPUT 9      // more output than ISIZE
#define INF_E_INPUT 10      // the deflate data runs past the member (BSIZE)
#define INF_E_TRAILING 11   // the deflate data ends before the member's trailer
#define INF_E_LENGTH 12     // less output than ISIZE
#define INF_E_CRC 13        // CRC32 of the output differs from the trailer
#define INF_E_ISIZE 14      // ISIZE above 64 KiB

#ifdef __HIP_DEVICE_COMPILE__
#define INF_SYNC() __syncthreads()
#define INF_UNI(x) ((unsigned)__builtin_amdgcn_readfirstlane((int)(x)))  // every lane holds the same value
#else
#define INF_SYNC() ((void)0)
#define INF_UNI(x) ((unsigned)(x))
#endif
#define INF_HD __host__ __device__ __forceinline__

struct InfTables {
    union {
        struct {
            uint16_t lfast[1 << INF_FAST_BITS];  // lit/len (and the code-length code): len << 9 | symbol, 0 = walk
            uint16_t dfast[1 << INF_FAST_BITS];
        } h;
        uint32_t crc[4][256];  // after decoding: slicing-by-4 CRC32 tables
    } u;
    uint32_t x2n[32];          // x^(2^k) mod P: the shift table that combines the lanes' CRCs
    uint32_t lane_crc[INF_THREADS];
    uint16_t lcount[16], dcount[16], offs[16];
    uint16_t lsym[288], dsym[32];
    uint8_t lens[320];
    uint8_t win[INF_WIN];
    uint32_t word;             // lane 0 -> everybody
};

struct InfBits {
    const uint8_t *in;
    uint32_t pos, end;     // next byte to load, end of the deflate data
    uint32_t wbase, wlen;  // the window holds in[wbase, wbase + wlen)
    uint32_t nbits;
    u64 buf;
};

INF_HD uint32_t inf_min(uint32_t a, uint32_t b) { return a < b ? a : b; }

// Tops the bit buffer up to more than 56 bits (or to the end of the data) from the LDS window.
INF_HD void inf_refill(InfBits &b, InfTables *t, unsigned lane, unsigned nl)
{
    while (b.nbits <= 56 && b.pos < b.end) {
        if (b.pos < b.wbase || b.pos >= b.wbase + b.wlen) {
            const uint32_t w = inf_min(INF_WIN, b.end - b.pos);
            INF_SYNC();  // everybody is done with the old window
            for (uint32_t i = lane; i < w; i += nl) t->win[i] = b.in[b.pos + i];
            INF_SYNC();
            b.wbase = b.pos;
            b.wlen = w;
        }
        const uint32_t k = inf_min((64 - b.nbits) >> 3, b.wbase + b.wlen - b.pos);
        for (uint32_t i = 0; i < k; ++i) {
            b.buf |= (u64)INF_UNI(t->win[b.pos - b.wbase + i]) << b.nbits;
            b.nbits += 8;
        }
        b.pos += k;
    }
}

INF_HD int inf_bits(InfBits &b, InfTables *t, unsigned lane, unsigned nl, unsigned n, uint32_t *v)
{
    if (b.nbits < n) {
        inf_refill(b, t, lane, nl);
        if (b.nbits < n) return INF_E_INPUT;
    }
    *v = (uint32_t)(b.buf & ((1ull << n) - 1));
    b.buf >>= n;
    b.nbits -= n;
    return 0;
}

// Canonical code of lens[0, n) -> count / sym and the first-level table.  Lane 0 counts and sorts, every lane fills
// table entries by walking the code with the entry's bits.  0, INF_E_OVERSUB or INF_E_INCOMPLETE (zlib's rule: an
// incomplete set is allowed only for a single code of length 1 outside the code-length code, or for no code at all).
INF_HD int inf_build(InfTables *t, const uint8_t *lens, unsigned n, uint16_t *count, uint16_t *sym, uint16_t *fast,
                     unsigned fbits, bool codes, unsigned lane, unsigned nl)
{
    INF_SYNC();  // lens written, the old table no longer read
    if (lane == 0) {
        for (int i = 0; i < 16; ++i) count[i] = 0;
        for (unsigned s = 0; s < n; ++s) ++count[lens[s]];
        int left = 1, maxlen = 0, err = 0;
        for (int len = 1; len < 16; ++len) {
            left = (left << 1) - count[len];
            if (left < 0) {
                err = INF_E_OVERSUB;
                break;
            }
            if (count[len]) maxlen = len;
        }
        if (!err && left > 0 && maxlen > 0 && (codes || maxlen != 1)) err = INF_E_INCOMPLETE;
        if (!err) {
            t->offs[1] = 0;
            for (int len = 1; len < 15; ++len) t->offs[len + 1] = t->offs[len] + count[len];
            for (unsigned s = 0; s < n; ++s)
                if (lens[s]) sym[t->offs[lens[s]]++] = (uint16_t)s;
        }
        t->word = err;
    }
    INF_SYNC();
    const int err = (int)INF_UNI(t->word);
    if (err) return err;
    for (unsigned e = lane; e < (1u << fbits); e += nl) {
        int code = 0, first = 0, index = 0;
        uint16_t entry = 0;
        for (unsigned len = 1; len <= fbits; ++len) {
            code |= (e >> (len - 1)) & 1;
            const int c = count[len];
            if (code - c < first) {
                entry = (uint16_t)(len << 9 | sym[index + code - first]);
                break;
            }
            index += c;
            first = (first + c) << 1;
            code <<= 1;
        }
        fast[e] = entry;
    }
    INF_SYNC();
    return 0;
}

INF_HD int inf_decode(InfBits &b, InfTables *t, const uint16_t *fast, const uint16_t *count, const uint16_t *sym,
                      unsigned fbits, unsigned lane, unsigned nl, unsigned *out)
{
    if (b.nbits < 15) inf_refill(b, t, lane, nl);
    const unsigned e = INF_UNI(fast[b.buf & ((1u << fbits) - 1)]);
    unsigned len = e >> 9, s = e & 511;
    if (!len) {  // longer than the table, or no code at all: walk the canonical code bit by bit
        int code = 0, first = 0, index = 0;
        for (unsigned l = 1; l < 16; ++l) {
            code |= (int)((b.buf >> (l - 1)) & 1);
            const int c = (int)INF_UNI(count[l]);
            if (code - c < first) {
                len = l;
                s = INF_UNI(sym[index + code - first]);
                break;
            }
            index += c;
            first = (first + c) << 1;
            code <<= 1;
        }
        if (!len) return b.nbits < 15 ? INF_E_INPUT : INF_E_CODE;
    }
    if (len > b.nbits) return INF_E_INPUT;
    b.buf >>= len;
    b.nbits -= len;
    *out = s;
    return 0;
}

// RFC 1951 3.2.5: length symbols 257..285, distance symbols 0..29
INF_HD void inf_len_code(unsigned c, unsigned *base, unsigned *extra)
{
    if (c == 28) *base = 258, *extra = 0;
    else if (c < 8) *base = 3 + c, *extra = 0;
    else *extra = (c - 4) >> 2, *base = ((4 + (c & 3)) << *extra) + 3;
}
INF_HD void inf_dist_code(unsigned c, unsigned *base, unsigned *extra)
{
    if (c < 4) *base = 1 + c, *extra = 0;
    else *extra = (c >> 1) - 1, *base = ((2 + (c & 1)) << *extra) + 1;
}
// the order of the code-length code lengths: 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
INF_HD unsigned inf_clen_order(unsigned i)
{
    if (i < 3) return 16 + i;
    if (i == 3) return 0;
    const unsigned k = i - 4;
    return (k & 1) ? 7 - (k >> 1) : 8 + (k >> 1);
}

// Dynamic block header: code lengths -> t->lens, then the lit/len and distance tables.
INF_HD int inf_dynamic(InfBits &b, InfTables *t, unsigned lane, unsigned nl)
{
    uint32_t hlit, hdist, hclen, v;
    int err;
    if ((err = inf_bits(b, t, lane, nl, 5, &hlit)) || (err = inf_bits(b, t, lane, nl, 5, &hdist)) ||
        (err = inf_bits(b, t, lane, nl, 4, &hclen)))
        return err;
    const unsigned nlen = hlit + 257, ndist = hdist + 1, ncode = hclen + 4;
    if (nlen > 286 || ndist > 30) return INF_E_LENS;
    INF_SYNC();
    for (unsigned i = lane; i < 19; i += nl) t->lens[i] = 0;
    INF_SYNC();
    for (unsigned i = 0; i < ncode; ++i) {
        if ((err = inf_bits(b, t, lane, nl, 3, &v))) return err;
        if (lane == 0) t->lens[inf_clen_order(i)] = (uint8_t)v;
    }
    if ((err = inf_build(t, t->lens, 19, t->lcount, t->lsym, t->u.h.lfast, 7, true, lane, nl))) return err;
    // the code lengths are decoded with the code-length code, which lives in the lit/len table until both are read
    unsigned i = 0, prev = 0;
    while (i < nlen + ndist) {
        unsigned s;
        if ((err = inf_decode(b, t, t->u.h.lfast, t->lcount, t->lsym, 7, lane, nl, &s))) return err;
        if (s < 16) {
            if (lane == 0) t->lens[i] = (uint8_t)s;
            prev = s;
            ++i;
            continue;
        }
        unsigned rep, val = 0;
        if (s == 16) {
            if (i == 0) return INF_E_LENS;
            if ((err = inf_bits(b, t, lane, nl, 2, &v))) return err;
            rep = 3 + v;
            val = prev;
        } else if (s == 17) {
            if ((err = inf_bits(b, t, lane, nl, 3, &v))) return err;
            rep = 3 + v;
        } else {
            if ((err = inf_bits(b, t, lane, nl, 7, &v))) return err;
            rep = 11 + v;
        }
        if (i + rep > nlen + ndist) return INF_E_LENS;
        for (unsigned k = lane; k < rep; k += nl) t->lens[i + k] = (uint8_t)val;
        prev = val;
        i += rep;
    }
    INF_SYNC();
    if (!INF_UNI(t->lens[256])) return INF_E_LENS;  // no end-of-block code
    if ((err = inf_build(t, t->lens, nlen, t->lcount, t->lsym, t->u.h.lfast, INF_FAST_BITS, false, lane, nl))) return err;
    return inf_build(t, t->lens + nlen, ndist, t->dcount, t->dsym, t->u.h.dfast, INF_FAST_BITS, false, lane, nl);
}

INF_HD int inf_fixed(InfTables *t, unsigned lane, unsigned nl)
{
    INF_SYNC();
    for (unsigned i = lane; i < 288 + 32; i += nl) t->lens[i] = i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : i < 288 ? 8 : 5;
    int err = inf_build(t, t->lens, 288, t->lcount, t->lsym, t->u.h.lfast, INF_FAST_BITS, false, lane, nl);
    if (!err) err = inf_build(t, t->lens + 288, 32, t->dcount, t->dsym, t->u.h.dfast, INF_FAST_BITS, false, lane, nl);
    return err;
}

// Symbols of one Huffman block until end-of-block.  Lane 0 writes literals; a match is copied by all lanes (a
// distance below its length repeats the pattern: byte j of the copy is out[pos - dist + j % dist]).
INF_HD int inf_codes(InfBits &b, InfTables *t, uint8_t *out, uint32_t isize, uint32_t *opos, unsigned lane, unsigned nl)
{
    uint32_t pos = *opos;
    int err = 0;
    for (;;) {
        unsigned s;
        if ((err = inf_decode(b, t, t->u.h.lfast, t->lcount, t->lsym, INF_FAST_BITS, lane, nl, &s))) break;
        if (s < 256) {
            if (pos >= isize) {
                err = INF_E_OUTPUT;
                break;
            }
            if (lane == 0) out[pos] = (uint8_t)s;
            ++pos;
            continue;
        }
        if (s == 256) break;
        if (s > 285) {
            err = INF_E_CODE;
            break;
        }
        unsigned base, extra, len, dist;
        uint32_t v = 0;
        inf_len_code(s - 257, &base, &extra);
        if (extra && (err = inf_bits(b, t, lane, nl, extra, &v))) break;
        len = base + v;
        if ((err = inf_decode(b, t, t->u.h.dfast, t->dcount, t->dsym, INF_FAST_BITS, lane, nl, &s))) break;
        if (s > 29) {
            err = INF_E_CODE;
            break;
        }
        inf_dist_code(s, &base, &extra);
        v = 0;
        if (extra && (err = inf_bits(b, t, lane, nl, extra, &v))) break;
        dist = base + v;
        if (dist > pos) {
            err = INF_E_DIST;
            break;
        }
        if (len > isize - pos) {
            err = INF_E_OUTPUT;
            break;
        }
        INF_SYNC();  // the bytes the copy reads are in LDS
        const uint8_t *src = out + pos - dist;
        if (dist >= len) {
            for (unsigned j = lane; j < len; j += nl) out[pos + j] = src[j];
        } else {
            for (unsigned j = lane; j < len; j += nl) out[pos + j] = src[j % dist];
        }
        pos += len;
    }
    *opos = pos;
    return err;
}

INF_HD uint32_t inf_rd32(const uint8_t *p) { return p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

// a * b modulo the CRC32 polynomial, both reflected (x^0 = bit 31)
INF_HD uint32_t inf_mulmod(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    for (int i = 31; i >= 0; --i) {
        if ((a >> i) & 1) p ^= b;
        b = (b & 1) ? (b >> 1) ^ 0xEDB88320u : b >> 1;
    }
    return p;
}

// CRC32 of out[0, n): lane k takes the k-th 4-byte-aligned chunk (slicing by 4), then
// crc(A || B) = crc(A) * x^(8 |B|) + crc(B) puts the chunks together; x^(8 |B|) comes from the table x^(2^k).
INF_HD uint32_t inf_crc32(InfTables *t, const uint8_t *out, uint32_t n, unsigned lane, unsigned nl)
{
    INF_SYNC();  // the Huffman tables are done with (the CRC tables share their space)
    for (unsigned i = lane; i < 256; i += nl) {
        uint32_t c = i;
        for (int k = 0; k < 8; ++k) c = (c & 1) ? (c >> 1) ^ 0xEDB88320u : c >> 1;
        t->u.crc[0][i] = c;
    }
    for (unsigned k = lane; k < 32; k += nl) {
        uint32_t x = 1u << 30;  // x^1
        for (unsigned j = 0; j < k; ++j) x = inf_mulmod(x, x);
        t->x2n[k] = x;
    }
    INF_SYNC();
    for (int j = 1; j < 4; ++j) {
        for (unsigned i = lane; i < 256; i += nl) {
            const uint32_t c = t->u.crc[j - 1][i];
            t->u.crc[j][i] = (c >> 8) ^ t->u.crc[0][c & 255];
        }
        INF_SYNC();
    }
    const uint32_t chunk = ((n + nl - 1) / nl + 3) & ~3u;
    uint32_t acc = 0;
    for (unsigned k = lane; k < nl; k += nl) {
        const uint32_t lo = inf_min(k * chunk, n), hi = inf_min(lo + chunk, n);
        uint32_t c = 0xFFFFFFFFu, i = lo;
        for (; i + 4 <= hi; i += 4) {
            c ^= *reinterpret_cast<const uint32_t *>(out + i);  // (lo is a multiple of 4, out is 16 B aligned)
            c = t->u.crc[3][c & 255] ^ t->u.crc[2][(c >> 8) & 255] ^ t->u.crc[1][(c >> 16) & 255] ^ t->u.crc[0][c >> 24];
        }
        for (; i < hi; ++i) c = (c >> 8) ^ t->u.crc[0][(c ^ out[i]) & 255];
        c = ~c;
        // shift by the bytes after this chunk: x^(8 m) = product of x^(2^(k+3)) over the set bits k of m
        uint32_t m = n - hi, x = 1u << 31;
        for (unsigned bit = 0; m; ++bit, m >>= 1)
            if (m & 1) x = inf_mulmod(x, t->x2n[bit + 3]);
        acc ^= inf_mulmod(x, c);
    }
    if (nl == 1) return acc;
    t->lane_crc[lane] = acc;
    INF_SYNC();
    uint32_t r = 0;
    for (unsigned k = 0; k < nl; ++k) r ^= t->lane_crc[k];
    return INF_UNI(r);
}

// One BGZF member in[0, in_size) -> out[0, isize) (out holds INF_OUT_MAX + 16 bytes, 16 B aligned).  Returns the status
// word (INF_E_* | bytes decoded << 8), the same in every lane.
INF_HD uint32_t inf_member(const uint8_t *in, uint32_t in_size, uint8_t *out, uint32_t isize, InfTables *t,
                           unsigned lane, unsigned nl)
{
    if (isize > INF_OUT_MAX) return INF_E_ISIZE;
    if (in_size < 18 || in[0] != 0x1F || in[1] != 0x8B || in[2] != 8 || (in[3] & 0xE0)) return INF_E_HEADER;
    const uint32_t flg = in[3], end = in_size - 8;
    uint32_t p = 10;
    if (flg & 4) p += 2 + (in[10] | (uint32_t)in[11] << 8);
    if (flg & 8) {  // FNAME, FCOMMENT: zero-terminated
        while (p < end && in[p]) ++p;
        ++p;
    }
    if (flg & 16) {
        while (p < end && in[p]) ++p;
        ++p;
    }
    if (flg & 2) p += 2;
    if (p > end) return INF_E_HEADER;

    InfBits b;
    b.in = in;
    b.pos = p;
    b.end = end;
    b.wbase = b.wlen = 0;
    b.nbits = 0;
    b.buf = 0;
    uint32_t opos = 0, bfinal = 0, btype = 0;
    int err = 0;
    while (!bfinal) {
        if ((err = inf_bits(b, t, lane, nl, 1, &bfinal)) || (err = inf_bits(b, t, lane, nl, 2, &btype))) break;
        if (btype == 0) {
            uint32_t len, nlen;
            b.buf >>= b.nbits & 7;  // to the byte border
            b.nbits &= ~7u;
            if ((err = inf_bits(b, t, lane, nl, 16, &len)) || (err = inf_bits(b, t, lane, nl, 16, &nlen))) break;
            if (len != (~nlen & 0xFFFF)) {
                err = INF_E_STORED;
                break;
            }
            b.pos -= b.nbits >> 3;  // give the prefetched bytes back
            b.nbits = 0;
            b.buf = 0;
            if (len > b.end - b.pos) {
                err = INF_E_INPUT;
                break;
            }
            if (len > isize - opos) {
                err = INF_E_OUTPUT;
                break;
            }
            for (uint32_t j = lane; j < len; j += nl) out[opos + j] = in[b.pos + j];
            b.pos += len;
            opos += len;
        } else if (btype == 3) {
            err = INF_E_BTYPE;
            break;
        } else {
            if ((err = btype == 1 ? inf_fixed(t, lane, nl) : inf_dynamic(b, t, lane, nl))) break;
            if ((err = inf_codes(b, t, out, isize, &opos, lane, nl))) break;
        }
    }
    if (!err && b.pos - (b.nbits >> 3) != end) err = INF_E_TRAILING;
    if (!err && opos != isize) err = INF_E_LENGTH;
    if (!err && inf_crc32(t, out, isize, lane, nl) != inf_rd32(in + end)) err = INF_E_CRC;
    return (uint32_t)err | opos << 8;
}

struct InfMember {
    unsigned in_off, in_size, out_off, isize;  // compressed bytes in the packed batch, text at out_off
};

// misc[3] = first failing member (none: 0xFFFFFFFF); mstat[i] = member i's status word
__global__ __launch_bounds__(INF_THREADS) void k_bgzf_inflate(const unsigned char *__restrict__ packed,
                                                              const InfMember *__restrict__ members,
                                                              unsigned char *__restrict__ text,
                                                              unsigned *__restrict__ mstat, unsigned *__restrict__ misc)
{
    __shared__ __attribute__((aligned(16))) unsigned char s_out[INF_OUT_MAX + 16];
    __shared__ InfTables s_t;
    const InfMember m = members[blockIdx.x];
    const unsigned lane = threadIdx.x;
    const uint32_t st = inf_member(packed + m.in_off, m.in_size, s_out, m.isize, &s_t, lane, INF_THREADS);
    if (lane == 0) mstat[blockIdx.x] = st;
    if (st & 255) {
        if (lane == 0) atomicMin(&misc[3], blockIdx.x);
        return;
    }
    __syncthreads();
    // out: head bytes up to a 16 B border of the text, then 16 B stores (assembled from LDS words), then the tail
    unsigned char *dst = text + m.out_off;
    const uint32_t n = m.isize;
    const uint32_t head = inf_min(n, (uint32_t)((16 - ((uintptr_t)dst & 15)) & 15));
    if (lane < head) dst[lane] = s_out[lane];
    const uint32_t nvec = (n - head) >> 4, sh = (head & 3) * 8;
    const unsigned *w = reinterpret_cast<const unsigned *>(s_out) + (head >> 2);
    for (uint32_t v = lane; v < nvec; v += INF_THREADS) {
        unsigned x[5];
#pragma unroll
        for (int j = 0; j < 5; ++j) x[j] = w[4 * v + j];
        v4u o;
        if (sh) {
            o.x = (x[0] >> sh) | (x[1] << (32 - sh));
            o.y = (x[1] >> sh) | (x[2] << (32 - sh));
            o.z = (x[2] >> sh) | (x[3] << (32 - sh));
            o.w = (x[3] >> sh) | (x[4] << (32 - sh));
        } else {
            o.x = x[0], o.y = x[1], o.z = x[2], o.w = x[3];
        }
        *reinterpret_cast<v4u *>(dst + head + 16 * v) = o;
    }
    for (uint32_t i = head + 16 * nvec + lane; i < n; i += INF_THREADS) dst[i] = s_out[i];
}

// The last batch: text[n] = '\n' when the final record has none, else 0 (the parser then sees n + 1 bytes).
__global__ void k_bgzf_finish(unsigned char *__restrict__ text, unsigned n)
{
    if (threadIdx.x == 0) text[n] = (n && text[n - 1] != '\n') ? '\n' : 0;
}

// misc[2] = max(misc[2], 1 + offset of the last '\n' in text[0, n))
__global__ __launch_bounds__(VCF_THREADS) void k_bgzf_last_nl(const unsigned char *__restrict__ text, unsigned n,
                                                              unsigned *__restrict__ misc)
{
    const unsigned cb = blockIdx.x * VCF_BLOCK_BYTES + threadIdx.x * 16;
    unsigned v = 0;
    if (cb < n) {
        const unsigned m = vcf_match16(*reinterpret_cast<const v4u *>(text + cb), '\n', cb, 0, n);
        if (m) v = cb + 32 - __clz(m);
    }
#pragma unroll
    for (int o = 32; o; o >>= 1) v = max(v, (unsigned)__shfl_xor((int)v, o));
    if ((threadIdx.x & 63) == 0 && v) atomicMax(&misc[2], v);
}
