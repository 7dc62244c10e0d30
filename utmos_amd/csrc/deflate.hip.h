// DEFLATE encoding on the GPU (RFC 1951, for the zlib stream of a joblib part file): the input is cut into 64 KiB
// segments that are compressed independently (fresh window, one block each), so the stream can be built by one
// workgroup per segment.  Every segment except the last ends byte-aligned with an empty stored block (what zlib's
// Z_SYNC_FLUSH emits); the last one sets BFINAL.
//
//   k_deflate_chain    one wave per segment: hash chains.  The segment is walked in rounds of DEF_ROUND
//                      positions; every position of a round reads the hash head left by the earlier rounds, then the
//                      round puts itself in with atomicMax (order-independent).  prev[p] = distance to that position.
//   k_deflate_match    one thread per position: the longest match among the chain's first `chain` candidates
//   k_deflate_parse    one wave per segment: the greedy (lazy from level 4) parse over the per-position matches, a
//                      serial walk over a 64-entry register window, tokens stored 64 at a time
//   k_deflate_encode   one workgroup per segment: Adler-32 sums, symbol histograms (LDS atomics), length-limited
//                      Huffman codes (lane 0), block size against stored blocks, then the bits: a prefix sum of the
//                      tokens' bit lengths and an OR of each token into an LDS window of words, flushed in order
//   k_deflate_scan     one workgroup: offsets of the segments' outputs in the batch's output (prefix sum of sizes)
//   k_deflate_gather   the segments' outputs packed back to back
//
// The segment stays in global memory (L2-resident); LDS holds only the hash heads (16 KiB) or the code tables and the
// bit window (about 10 KiB).  Every race resolves by max or OR, and every loop is over positions, tokens or symbols, not
// lanes, so the bytes do not depend on the schedule or on the lane count: the functions below are __host__ __device__,
// and utm_deflate_host runs them with one lane to produce the same bytes on the CPU.
//
// Levels (search effort; the format does not change):
//   level        1    2    3    4    5    6    7    8    9
//   candidates   2    4    8   16   32   64  128  256  512   (per position, along the hash chain)
//   nice length 32   32  128  128  128  258  258  258  258   (a match this long ends the search)
//   lazy         -    -    -  yes  yes  yes  yes  yes  yes   (literal when the next position has a longer match)
#pragma once
#include "common.hip.h"

#define DEF_SEG 65536u      // input bytes per segment (one workgroup, one block)
#define DEF_WIN 32768u      // LZ77 window
#define DEF_ROUND 64u       // positions per hash round (a match whose source is in the same round is not seen)
#define DEF_HBITS 12
#define DEF_HSIZE (1u << DEF_HBITS)
#define DEF_THREADS 256
#define DEF_CHUNK 256u      // tokens per emission step
#define DEF_BUFW 512u       // LDS bit window in words: the dynamic header (< 5,000 bits) or a chunk (<= 256 x 48 bits)
#define DEF_SEG_OUT 65600u  // output room per segment: stored blocks take at most n + 15 bytes
#define DEF_PAD 16u         // readable bytes after the input (word loads past the last byte)
#define DEF_ADLER_MOD 65521u

#ifdef __HIP_DEVICE_COMPILE__
#define DEF_SYNC() __syncthreads()
#define DEF_AMAX(p, v) atomicMax((p), (v))
#define DEF_AOR(p, v) atomicOr((p), (v))
#define DEF_AADD(p, v) atomicAdd((p), (v))
#else
#define DEF_SYNC() ((void)0)
#define DEF_AMAX(p, v) (*(p) = *(p) > (v) ? *(p) : (v))
#define DEF_AOR(p, v) (*(p) |= (v))
#define DEF_AADD(p, v) (*(p) += (v))
#endif
#define DEF_HD __host__ __device__ __forceinline__

struct DefLevel {
    uint32_t chain, nice;
    bool lazy;
};

DEF_HD DefLevel def_level(int level)
{
    DefLevel l;
    l.chain = 1u << level;
    l.nice = level <= 2 ? 32 : level <= 5 ? 128 : 258;
    l.lazy = level >= 4;
    return l;
}

DEF_HD uint32_t def_min(uint32_t a, uint32_t b) { return a < b ? a : b; }

// 4 bytes at in + i from aligned words (in is 4-byte aligned and readable DEF_PAD bytes past the segment)
DEF_HD uint32_t def_ld32(const uint8_t *in, uint32_t i)
{
    const uint32_t *w = reinterpret_cast<const uint32_t *>(in) + (i >> 2);
    const uint32_t s = (i & 3) * 8;
    return s ? (w[0] >> s) | (w[1] << (32 - s)) : w[0];
}

DEF_HD uint32_t def_hash(const uint8_t *in, uint32_t p) { return ((def_ld32(in, p) & 0xFFFFFFu) * 2654435761u) >> (32 - DEF_HBITS); }

// prev[p] = p - (the last position q before p's round with the hash of p), 0 when there is none within the window.
// head: DEF_HSIZE words (q + 1, 0 = none).
DEF_HD void def_chain(const uint8_t *in, uint32_t n, uint16_t *prev, uint32_t *head, unsigned lane, unsigned nl)
{
    for (uint32_t i = lane; i < DEF_HSIZE; i += nl) head[i] = 0;
    DEF_SYNC();
    for (uint32_t r = 0; r < n; r += DEF_ROUND) {
        const uint32_t m = def_min(DEF_ROUND, n - r);
        for (uint32_t i = lane; i < m; i += nl) {
            const uint32_t p = r + i;
            uint32_t d = 0;
            if (p + 3 <= n) {
                const uint32_t q1 = head[def_hash(in, p)];
                if (q1 && p - (q1 - 1) <= DEF_WIN) d = p - (q1 - 1);
            }
            prev[p] = (uint16_t)d;
        }
        DEF_SYNC();
        for (uint32_t i = lane; i < m; i += nl) {
            const uint32_t p = r + i;
            if (p + 3 <= n) DEF_AMAX(&head[def_hash(in, p)], p + 1);
        }
        DEF_SYNC();
    }
}

// The longest match for position p (len << 16 | distance), 0 when there is none worth coding: length >= 3, the
// first of equal lengths along the chain (the nearest), a length-3 match only within 4 KiB.
DEF_HD uint32_t def_match(const uint8_t *in, uint32_t n, const uint16_t *prev, uint32_t p, DefLevel lv)
{
    if (p + 3 > n) return 0;
    const uint32_t maxlen = def_min(258, n - p), nice = def_min(lv.nice, maxlen);
    uint32_t best = 2, bestd = 0, q = p, d = prev[p];
    for (uint32_t c = 0; c < lv.chain && d; ++c) {
        q -= d;
        if (p - q > DEF_WIN) break;
        d = prev[q];
        if (in[q + best] != in[p + best] || in[q] != in[p]) continue;  // (best < maxlen: the search stops at nice)
        uint32_t len = 0;
        for (;;) {
            const uint32_t x = def_ld32(in, p + len) ^ def_ld32(in, q + len);
            if (x) {
                len += (uint32_t)__builtin_ctz(x) >> 3;
                break;
            }
            len += 4;
            if (len >= maxlen) break;
        }
        len = def_min(len, maxlen);
        if (len > best) {
            best = len;
            bestd = p - q;
            if (len >= nice) break;
        }
    }
    if (!bestd || (best == 3 && bestd > 4096)) return 0;
    return best << 16 | bestd;
}

// One parse step at p: the token (len << 16 | dist for a match, the byte for a literal) and its length in bytes.
// cur = the match at p, next = the match at p + 1 (used when lazy).
DEF_HD uint32_t def_step(uint32_t cur, uint32_t next, uint32_t byte, bool lazy, uint32_t *adv)
{
    const uint32_t len = cur >> 16;
    if (len && !(lazy && (next >> 16) > len)) {
        *adv = len;
        return cur;
    }
    *adv = 1;
    return byte;
}

// RFC 1951 3.2.5: length 3..258 -> symbol 257..285 and its extra bits; distance 1..32768 -> symbol 0..29
DEF_HD uint32_t def_len_sym(uint32_t len, uint32_t *extra, uint32_t *ebits)
{
    if (len == 258) {
        *ebits = 0, *extra = 0;
        return 285;
    }
    const uint32_t l = len - 3;
    if (l < 8) {
        *ebits = 0, *extra = 0;
        return 257 + l;
    }
    const uint32_t hb = 31 - __builtin_clz(l);  // 3..7
    const uint32_t eb = hb - 2;
    *ebits = eb;
    *extra = l & ((1u << eb) - 1);
    return 257 + 4 * eb + 4 + ((l >> eb) & 3);
}
DEF_HD uint32_t def_dist_sym(uint32_t dist, uint32_t *extra, uint32_t *ebits)
{
    const uint32_t d = dist - 1;
    if (d < 4) {
        *ebits = 0, *extra = 0;
        return d;
    }
    const uint32_t hb = 31 - __builtin_clz(d);  // 2..14
    const uint32_t eb = hb - 1;
    *ebits = eb;
    *extra = d & ((1u << eb) - 1);
    return 2 * hb + ((d >> eb) & 1);
}

struct DefTables {
    uint32_t lfreq[288], dfreq[32], cfreq[19];
    uint32_t work[288];            // Huffman lengths by rank (Moffat-Katajainen in place)
    uint16_t sorted[288];          // used symbols by (frequency, symbol)
    uint16_t lcode[288], dcode[32], ccode[19];  // bit-reversed canonical codes
    uint8_t llen[288], dlen[32], clen[19];
    uint8_t all[320];              // the lit/len and distance code lengths back to back
    uint8_t rle[320], rlex[320];   // ... run-length coded (symbols 0..18, extra values)
    uint32_t cnt[16], next[16];    // lengths per count, next canonical code per length
    uint32_t buf[DEF_BUFW + 4];    // bit window: buf[0] holds stream bits [32 wbase, ...)
    uint32_t scan[DEF_CHUNK];
    uint32_t adler[2][DEF_THREADS];
    uint32_t word[8];              // lane 0 -> everybody
};

// Code lengths (at most `limit` bits) for freq[0, n) into len[0, n): Huffman by Moffat-Katajainen on the symbols sorted
// by (frequency, symbol), then lengths above the limit folded back with the Kraft sum kept at 1.  Fewer than two used
// symbols get two codes of length 1 (symbols 0 and 1 if needed), as zlib does.  Every lane calls it.
DEF_HD void def_huffman(DefTables *t, const uint32_t *freq_in, unsigned n, unsigned limit, uint8_t *len, unsigned lane,
                        unsigned nl)
{
    DEF_SYNC();
    if (lane == 0) {
        unsigned used = 0;
        for (unsigned s = 0; s < n; ++s) used += freq_in[s] != 0;
        t->word[0] = used;
    }
    DEF_SYNC();
    const unsigned used0 = t->word[0];
    // the frequencies the code is built for: zero-frequency symbols 0 / 1 become 1 while fewer than two are used
    auto fq = [&](unsigned s) -> uint32_t {
        const uint32_t f = freq_in[s];
        if (f || used0 >= 2 || s > 1) return f;
        if (used0 == 0) return 1;
        return (s == 0 || freq_in[0] != 0) ? 1 : 0;  // one used: symbol 0, or symbol 1 when 0 is the used one
    };
    for (unsigned s = lane; s < n; s += nl) {
        const uint32_t f = fq(s);
        len[s] = 0;
        if (!f) continue;
        unsigned r = 0;
        for (unsigned u = 0; u < n; ++u) {
            const uint32_t g = fq(u);
            r += g && (g < f || (g == f && u < s));
        }
        t->sorted[r] = (uint16_t)s;
    }
    DEF_SYNC();
    if (lane == 0) {
        unsigned m = 0;
        for (unsigned s = 0; s < n; ++s) m += fq(s) != 0;
        uint32_t *A = t->work;
        for (unsigned i = 0; i < m; ++i) A[i] = fq(t->sorted[i]);
        // in-place minimum-redundancy code lengths (A ascending -> A[i] = depth of leaf i)
        int root = 0, leaf = 2, next;
        A[0] += A[1];
        for (next = 1; next < (int)m - 1; ++next) {
            if (leaf >= (int)m || A[root] < A[leaf]) {
                A[next] = A[root];
                A[root++] = next;
            } else {
                A[next] = A[leaf++];
            }
            if (leaf >= (int)m || (root < next && A[root] < A[leaf])) {
                A[next] += A[root];
                A[root++] = next;
            } else {
                A[next] += A[leaf++];
            }
        }
        A[m - 2] = 0;
        for (next = (int)m - 3; next >= 0; --next) A[next] = A[A[next]] + 1;
        int avail = 1, nused = 0, depth = 0;
        root = (int)m - 2;
        next = (int)m - 1;
        while (avail > 0) {
            while (root >= 0 && (int)A[root] == depth) {
                ++nused;
                --root;
            }
            while (avail > nused) {
                A[next--] = depth;
                --avail;
            }
            avail = 2 * nused;
            ++depth;
            nused = 0;
        }
        // lengths per count, longer than the limit folded to the limit, then the Kraft sum brought back to 1
        uint32_t *cnt = t->cnt;
        for (unsigned l = 0; l < 16; ++l) cnt[l] = 0;
        for (unsigned i = 0; i < m; ++i) ++cnt[A[i] > limit ? limit : A[i]];
        uint32_t total = 0;
        for (unsigned l = 1; l <= limit; ++l) total += cnt[l] << (limit - l);
        while (total > (1u << limit)) {
            --cnt[limit];
            for (unsigned l = limit - 1; l > 0; --l)
                if (cnt[l]) {
                    --cnt[l];
                    cnt[l + 1] += 2;
                    break;
                }
            --total;
        }
        // the most frequent symbols take the shortest lengths
        unsigned i = m;
        for (unsigned l = 1; l <= limit; ++l)
            for (uint32_t k = 0; k < cnt[l]; ++k) len[t->sorted[--i]] = (uint8_t)l;
    }
    DEF_SYNC();
}

// Canonical codes of len[0, n), bit-reversed for the LSB-first stream (lane 0).
DEF_HD void def_codes(DefTables *t, const uint8_t *len, unsigned n, uint16_t *code)
{
    uint32_t *cnt = t->cnt, *next = t->next;
    for (unsigned l = 0; l < 16; ++l) cnt[l] = 0;
    for (unsigned s = 0; s < n; ++s) ++cnt[len[s]];
    cnt[0] = 0;
    uint32_t c = 0;
    for (unsigned l = 1; l < 16; ++l) {
        c = (c + cnt[l - 1]) << 1;
        next[l] = c;
    }
    for (unsigned s = 0; s < n; ++s) {
        const unsigned l = len[s];
        code[s] = 0;
        if (!l) continue;
        const uint32_t v = next[l]++;
        uint32_t r = 0;
        for (unsigned k = 0; k < l; ++k) r |= ((v >> k) & 1) << (l - 1 - k);
        code[s] = (uint16_t)r;
    }
}

// ORs nbits (<= 57) of v into the window at stream bit `bit` (the window starts at bit 32 * wbase).
DEF_HD void def_put(uint32_t *buf, u64 bit, u64 wbase, u64 v, unsigned nbits, bool atomic)
{
    if (!nbits) return;
    const uint32_t w = (uint32_t)((bit >> 5) - wbase), s = (uint32_t)(bit & 31);
    const u64 lo = v << s, hi = s ? v >> (64 - s) : 0;
    const uint32_t p0 = (uint32_t)lo, p1 = (uint32_t)(lo >> 32), p2 = (uint32_t)hi;
    if (atomic) {
        if (p0) DEF_AOR(&buf[w], p0);
        if (p1) DEF_AOR(&buf[w + 1], p1);
        if (p2) DEF_AOR(&buf[w + 2], p2);
    } else {
        buf[w] |= p0, buf[w + 1] |= p1, buf[w + 2] |= p2;
    }
}

// The bits of one token and their count (lit/len code, length extra, distance code, distance extra).
DEF_HD u64 def_token_bits(const DefTables *t, uint32_t tok, unsigned *nbits)
{
    const uint32_t len = tok >> 16;
    if (!len) {
        *nbits = t->llen[tok];
        return t->lcode[tok];
    }
    uint32_t le, lb, de, db;
    const uint32_t ls = def_len_sym(len, &le, &lb), ds = def_dist_sym(tok & 0xFFFF, &de, &db);
    unsigned n = t->llen[ls];
    u64 v = t->lcode[ls];
    v |= (u64)le << n;
    n += lb;
    v |= (u64)t->dcode[ds] << n;
    n += t->dlen[ds];
    v |= (u64)de << n;
    n += db;
    *nbits = n;
    return v;
}

// Full words of the window [0, upto) to out + 4 * wbase, the partial word moved to the front, the rest zeroed.
DEF_HD void def_flush(DefTables *t, uint8_t *out, u64 *wbase, u64 bit_end, unsigned lane, unsigned nl)
{
    const uint32_t full = (uint32_t)((bit_end >> 5) - *wbase);
    uint32_t *dst = reinterpret_cast<uint32_t *>(out) + *wbase;
    DEF_SYNC();
    for (uint32_t i = lane; i < full; i += nl)
        if (*wbase + i < DEF_SEG_OUT / 4) dst[i] = t->buf[i];  // (the size check keeps the block inside the region)
    DEF_SYNC();
    const uint32_t keep = t->buf[full];
    DEF_SYNC();
    for (uint32_t i = lane; i < DEF_BUFW + 4; i += nl) t->buf[i] = i == 0 ? keep : 0;
    DEF_SYNC();
    *wbase += full;
}

// One segment: in[0, n) (4-byte aligned, readable DEF_PAD bytes further), tok[0, ntok) from the parse -> out (4-byte
// aligned, DEF_SEG_OUT bytes).  Returns the segment's output bytes; adler[0] = sum of the bytes mod 65521, adler[1] =
// sum of (n - i) * byte i mod 65521 (the segment's share of the running Adler-32).
DEF_HD uint32_t def_encode(const uint8_t *in, uint32_t n, const uint32_t *tok, uint32_t ntok, bool last, uint8_t *out,
                           uint32_t *adler, DefTables *t, unsigned lane, unsigned nl)
{
    // Adler-32 sums: any split of the bytes gives the same sums modulo 65521
    {
        const uint32_t chunk = (n + nl - 1) / nl, lo = def_min(lane * chunk, n), hi = def_min(lo + chunk, n);
        u64 s1 = 0, s2 = 0;
        for (uint32_t i = lo; i < hi; ++i) {
            s1 += in[i];
            s2 += (u64)(hi - i) * in[i];
        }
        t->adler[0][lane] = (uint32_t)(s1 % DEF_ADLER_MOD);
        t->adler[1][lane] = (uint32_t)((s2 + (u64)(n - hi) * s1) % DEF_ADLER_MOD);
    }
    for (unsigned s = lane; s < 288; s += nl) t->lfreq[s] = 0;
    for (unsigned s = lane; s < 32; s += nl) t->dfreq[s] = 0;
    for (unsigned s = lane; s < 19; s += nl) t->cfreq[s] = 0;
    DEF_SYNC();
    if (lane == 0) {
        u64 a = 0, b = 0;
        for (unsigned k = 0; k < nl; ++k) a += t->adler[0][k], b += t->adler[1][k];
        adler[0] = (uint32_t)(a % DEF_ADLER_MOD);
        adler[1] = (uint32_t)(b % DEF_ADLER_MOD);
        t->lfreq[256] = 1;
    }
    for (uint32_t i = lane; i < ntok; i += nl) {
        const uint32_t tk = tok[i], len = tk >> 16;
        if (!len) {
            DEF_AADD(&t->lfreq[tk], 1u);
        } else {
            uint32_t e, b;
            DEF_AADD(&t->lfreq[def_len_sym(len, &e, &b)], 1u);
            DEF_AADD(&t->dfreq[def_dist_sym(tk & 0xFFFF, &e, &b)], 1u);
        }
    }
    def_huffman(t, t->lfreq, 286, 15, t->llen, lane, nl);
    def_huffman(t, t->dfreq, 30, 15, t->dlen, lane, nl);
    // lane 0: the code-length code, the block's size in bits, stored or not
    if (lane == 0) {
        def_codes(t, t->llen, 286, t->lcode);
        def_codes(t, t->dlen, 30, t->dcode);
        unsigned nlit = 286, ndist = 30;
        while (nlit > 257 && !t->llen[nlit - 1]) --nlit;
        while (ndist > 1 && !t->dlen[ndist - 1]) --ndist;
        uint8_t *all = t->all;
        for (unsigned s = 0; s < nlit; ++s) all[s] = t->llen[s];
        for (unsigned s = 0; s < ndist; ++s) all[nlit + s] = t->dlen[s];
        const unsigned na = nlit + ndist;
        unsigned nr = 0;
        for (unsigned i = 0; i < na;) {
            const uint8_t v = all[i];
            unsigned run = 1;
            while (i + run < na && all[i + run] == v) ++run;
            i += run;
            if (v == 0) {
                while (run >= 11) {
                    const unsigned r = run < 138 ? run : 138;
                    t->rle[nr] = 18, t->rlex[nr++] = (uint8_t)(r - 11);
                    run -= r;
                }
                if (run >= 3) {
                    t->rle[nr] = 17, t->rlex[nr++] = (uint8_t)(run - 3);
                    run = 0;
                }
            } else {
                t->rle[nr] = v, t->rlex[nr++] = 0;
                --run;
                while (run >= 3) {
                    const unsigned r = run < 6 ? run : 6;
                    t->rle[nr] = 16, t->rlex[nr++] = (uint8_t)(r - 3);
                    run -= r;
                }
            }
            for (; run; --run) t->rle[nr] = v, t->rlex[nr++] = 0;
        }
        for (unsigned i = 0; i < nr; ++i) ++t->cfreq[t->rle[i]];
        t->word[1] = nlit;
        t->word[2] = ndist;
        t->word[3] = nr;
    }
    def_huffman(t, t->cfreq, 19, 7, t->clen, lane, nl);
    if (lane == 0) {
        def_codes(t, t->clen, 19, t->ccode);
        unsigned hclen = 19;
        while (hclen > 4 && !t->clen[inf_clen_order(hclen - 1)]) --hclen;
        u64 bits = 3 + 14 + 3 * hclen;
        for (unsigned i = 0; i < t->word[3]; ++i) {
            const unsigned s = t->rle[i];
            bits += t->clen[s] + (s == 16 ? 2 : s == 17 ? 3 : s == 18 ? 7 : 0);
        }
        for (unsigned s = 0; s < 286; ++s) {
            const unsigned eb = (s >= 265 && s < 285) ? (s - 261) >> 2 : 0;
            bits += (u64)t->lfreq[s] * (t->llen[s] + eb);
        }
        for (unsigned s = 0; s < 30; ++s) bits += (u64)t->dfreq[s] * (t->dlen[s] + (s >= 4 ? (s >> 1) - 1 : 0));
        const u64 dyn = last ? (bits + 7) / 8 : (bits + 3 + 7) / 8 + 4;
        const uint32_t nblk = n ? (n + 65534) / 65535 : 1;
        const u64 stored = (u64)n + 5 * nblk + (last ? 0 : 5);
        t->word[4] = stored <= dyn;
        t->word[5] = hclen;
    }
    DEF_SYNC();
    if (t->word[4]) {  // stored blocks of at most 65,535 bytes, then the empty one
        const uint32_t nblk = n ? (n + 65534) / 65535 : 1;
        for (uint32_t i = lane; i < n; i += nl) {
            const uint32_t b = i / 65535;
            out[i + 5 * (b + 1)] = in[i];
        }
        for (uint32_t b = lane; b < nblk; b += nl) {
            const uint32_t len = def_min(65535, n - b * 65535);
            uint8_t *h = out + b * 65535 + 5 * b;
            h[0] = (last && b == nblk - 1) ? 1 : 0;
            h[1] = (uint8_t)len, h[2] = (uint8_t)(len >> 8), h[3] = (uint8_t)~len, h[4] = (uint8_t)(~len >> 8);
        }
        const uint32_t end = n + 5 * nblk;
        if (!last && lane == 0) out[end] = 0, out[end + 1] = 0, out[end + 2] = 0, out[end + 3] = 0xFF, out[end + 4] = 0xFF;
        DEF_SYNC();
        return end + (last ? 0 : 5);
    }
    // the dynamic block: header by lane 0, then the tokens DEF_CHUNK at a time
    for (uint32_t i = lane; i < DEF_BUFW + 4; i += nl) t->buf[i] = 0;
    DEF_SYNC();
    u64 bit = 0, wbase = 0;
    if (lane == 0) {
        const unsigned nlit = t->word[1], ndist = t->word[2], nr = t->word[3], hclen = t->word[5];
        def_put(t->buf, bit, 0, last ? 5 : 4, 3, false);  // BFINAL, BTYPE 2
        bit += 3;
        def_put(t->buf, bit, 0, (nlit - 257) | (ndist - 1) << 5 | (hclen - 4) << 10, 14, false);
        bit += 14;
        for (unsigned i = 0; i < hclen; ++i, bit += 3) def_put(t->buf, bit, 0, t->clen[inf_clen_order(i)], 3, false);
        for (unsigned i = 0; i < nr; ++i) {
            const unsigned s = t->rle[i], eb = s == 16 ? 2 : s == 17 ? 3 : s == 18 ? 7 : 0;
            def_put(t->buf, bit, 0, t->ccode[s] | (u64)t->rlex[i] << t->clen[s], t->clen[s] + eb, false);
            bit += t->clen[s] + eb;
        }
        t->word[6] = (uint32_t)bit;
    }
    DEF_SYNC();
    bit = t->word[6];
    def_flush(t, out, &wbase, bit, lane, nl);
    for (uint32_t c = 0; c < ntok; c += DEF_CHUNK) {
        const uint32_t m = def_min(DEF_CHUNK, ntok - c);
        for (uint32_t i = lane; i < DEF_CHUNK; i += nl) {
            unsigned nb = 0;
            if (i < m) def_token_bits(t, tok[c + i], &nb);
            t->scan[i] = nb;
        }
        // inclusive prefix sum of the bit counts (device: Hillis-Steele, one entry per lane; CPU: serially)
#ifdef __HIP_DEVICE_COMPILE__
        for (uint32_t d = 1; d < DEF_CHUNK; d <<= 1) {
            __syncthreads();
            const uint32_t x = lane >= d ? t->scan[lane - d] : 0;
            __syncthreads();
            t->scan[lane] += x;
        }
#else
        for (uint32_t i = 1; i < DEF_CHUNK; ++i) t->scan[i] += t->scan[i - 1];
#endif
        DEF_SYNC();
        for (uint32_t i = lane; i < m; i += nl) {
            unsigned nb;
            const u64 v = def_token_bits(t, tok[c + i], &nb);
            def_put(t->buf, bit + t->scan[i] - nb, wbase, v, nb, true);
        }
        bit += t->scan[m - 1];
        def_flush(t, out, &wbase, bit, lane, nl);
    }
    if (lane == 0) {  // end of block; not the last segment: an empty stored block to the byte border
        def_put(t->buf, bit, wbase, t->lcode[256], t->llen[256], false);
        bit += t->llen[256];
        if (!last) {
            bit += 3;  // BFINAL 0, BTYPE 0
            bit = (bit + 7) & ~7ull;
            def_put(t->buf, bit, wbase, 0xFFFF0000u, 32, false);
            bit += 32;
        }
        bit = (bit + 7) & ~7ull;
        t->word[7] = (uint32_t)bit;
    }
    DEF_SYNC();
    bit = t->word[7];
    def_flush(t, out, &wbase, bit + 31, lane, nl);
    return (uint32_t)(bit >> 3);
}

// ---- kernels ----------------------------------------------------------------------------------------------------

__device__ __forceinline__ uint32_t def_seg_len(uint32_t seg, uint32_t n) { return def_min(DEF_SEG, n - seg * DEF_SEG); }

// one wave per segment (a round is DEF_ROUND = 64 positions)
__global__ __launch_bounds__(DEF_ROUND) void k_deflate_chain(const uint8_t *__restrict__ in, uint32_t n,
                                                             uint16_t *__restrict__ prev)
{
    __shared__ uint32_t s_head[DEF_HSIZE];
    const uint32_t base = blockIdx.x * DEF_SEG;
    def_chain(in + base, def_seg_len(blockIdx.x, n), prev + base, s_head, threadIdx.x, DEF_ROUND);
}

// grid: (DEF_SEG / DEF_THREADS, segments)
__global__ __launch_bounds__(DEF_THREADS) void k_deflate_match(const uint8_t *__restrict__ in, uint32_t n,
                                                               const uint16_t *__restrict__ prev,
                                                               uint32_t *__restrict__ match, int level)
{
    const uint32_t base = blockIdx.y * DEF_SEG, len = def_seg_len(blockIdx.y, n);
    const uint32_t p = blockIdx.x * DEF_THREADS + threadIdx.x;
    if (p < len) match[base + p] = def_match(in + base, len, prev + base, p, def_level(level));
}

// One wave per segment: tokens to tok[seg * DEF_SEG ...], their count to ntok[seg].
__global__ __launch_bounds__(64) void k_deflate_parse(const uint8_t *__restrict__ in, uint32_t n,
                                                      const uint32_t *__restrict__ match, uint32_t *__restrict__ tok,
                                                      uint32_t *__restrict__ ntok, int level)
{
    const uint32_t base = blockIdx.x * DEF_SEG, len = def_seg_len(blockIdx.x, n);
    const unsigned lane = threadIdx.x;
    const bool lazy = def_level(level).lazy;
    const uint32_t *m = match + base;
    const uint8_t *src = in + base;
    uint32_t *out = tok + base;
    uint32_t p = 0, k = 0, mine = 0;
    while (p < len) {
        const uint32_t w0 = p, lim = def_min(w0 + 64, len);
        const uint32_t wm = w0 + lane < len ? m[w0 + lane] : 0, wb = w0 + lane < len ? src[w0 + lane] : 0;
        while (p < lim) {
            if (lazy && p + 1 == lim && lim < len) break;  // the next match is outside the window: reload at p
            const uint32_t i = p - w0;
            const uint32_t cur = (uint32_t)__shfl((int)wm, (int)i), byte = (uint32_t)__shfl((int)wb, (int)i);
            const uint32_t nxt = p + 1 < lim ? (uint32_t)__shfl((int)wm, (int)i + 1) : 0;
            uint32_t adv;
            const uint32_t t = def_step(cur, nxt, byte, lazy, &adv);
            if (lane == (k & 63)) mine = t;
            if ((++k & 63) == 0) out[k - 64 + lane] = mine;
            p += adv;
        }
    }
    if (lane < (k & 63)) out[(k & ~63u) + lane] = mine;
    if (lane == 0) ntok[blockIdx.x] = k;
}

// sizes[seg] = output bytes, adler[2 seg ..] = the segment's Adler-32 sums; output in seg_out + seg * DEF_SEG_OUT.
__global__ __launch_bounds__(DEF_THREADS) void k_deflate_encode(const uint8_t *__restrict__ in, uint32_t n,
                                                                const uint32_t *__restrict__ tok,
                                                                const uint32_t *__restrict__ ntok, int last_seg,
                                                                uint8_t *__restrict__ seg_out,
                                                                uint32_t *__restrict__ sizes,
                                                                uint32_t *__restrict__ adler)
{
    __shared__ DefTables s_t;
    const uint32_t seg = blockIdx.x, base = seg * DEF_SEG;
    const uint32_t bytes = def_encode(in + base, def_seg_len(seg, n), tok + base, ntok[seg], (int)seg == last_seg,
                                      seg_out + (u64)seg * DEF_SEG_OUT, adler + 2 * seg, &s_t, threadIdx.x, DEF_THREADS);
    if (threadIdx.x == 0) sizes[seg] = bytes;
}

// offs[0, nseg] = exclusive prefix sum of sizes (offs[nseg] = the batch's output bytes)
__global__ __launch_bounds__(DEF_THREADS) void k_deflate_scan(const uint32_t *__restrict__ sizes, uint32_t nseg,
                                                              uint32_t *__restrict__ offs)
{
    __shared__ uint32_t s[DEF_THREADS];
    uint32_t carry = 0;
    for (uint32_t c = 0; c < nseg; c += DEF_THREADS) {
        const uint32_t i = c + threadIdx.x;
        uint32_t v = i < nseg ? sizes[i] : 0;
        s[threadIdx.x] = v;
        for (uint32_t d = 1; d < DEF_THREADS; d <<= 1) {
            __syncthreads();
            const uint32_t x = threadIdx.x >= d ? s[threadIdx.x - d] : 0;
            __syncthreads();
            s[threadIdx.x] += x;
        }
        __syncthreads();
        if (i < nseg) offs[i] = carry + s[threadIdx.x] - v;
        carry += s[DEF_THREADS - 1];
        __syncthreads();
    }
    if (threadIdx.x == 0) offs[nseg] = carry;
}

// grid: (segments): the segment's bytes to out + offs[seg]
__global__ __launch_bounds__(DEF_THREADS) void k_deflate_gather(const uint8_t *__restrict__ seg_out,
                                                                const uint32_t *__restrict__ sizes,
                                                                const uint32_t *__restrict__ offs,
                                                                uint8_t *__restrict__ out)
{
    const uint32_t seg = blockIdx.x, n = sizes[seg];
    const uint32_t *src = reinterpret_cast<const uint32_t *>(seg_out + (u64)seg * DEF_SEG_OUT);
    uint8_t *dst = out + offs[seg];
    for (uint32_t w = threadIdx.x; 4 * w < n; w += DEF_THREADS) {
        const uint32_t v = src[w], m = def_min(4, n - 4 * w);
        for (uint32_t k = 0; k < m; ++k) dst[4 * w + k] = (uint8_t)(v >> (8 * k));
    }
}
