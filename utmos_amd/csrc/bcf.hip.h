// BCF2 genotype parsing on the GPU: the bytes of a BCF stream after its header -> the same per-record outputs as
// vcf.hip.h (packed presence row, AF, het / hom-alt counts, singleton flag; utmos/convert.py:43-88, restated on the CPU
// by utmos_amd/bcfio.py).  The format subset is DESIGN §8.4.
//
//   k_bcf_chain   one workgroup: follows the records' length prefixes (8 + l_shared + l_indiv) through the batch ->
//                 the offset of every whole record, their count, and where the unfinished rest (the carry) starts.
//                 All lanes stage a window of the text into LDS, one lane hops through it, all lanes flush the offsets.
//   k_bcf_parse   one 256-thread workgroup per record: the counts of the shared block, the walk over the FORMAT field
//                 headers to the GT key, then the cells -- a fast path for int8 diploid vectors (16 B = 8 samples = one
//                 output byte per lane), a general path (one sample per lane) for every other width and length.
//
// Records start at any byte.  Nothing here relies on unaligned global loads: single values are assembled from byte loads,
// and the fast path assembles its 16 genotype bytes from two aligned 16 B loads.  The text buffer is readable 64 B past
// its end (VCF_TEXT_PAD), so the second of those loads never leaves it.  Offsets are 32-bit as in vcf.hip.h.
//
// bcf_hop, bcf_find_gt and bcf_cell are __host__ __device__: utm_bcf_parse_host (host_bcf.hip.h) runs the same code on
// the CPU, one record after the other.
#pragma once
#include "vcf.hip.h"

#define BCF_WINDOW 32768u    // LDS window of the chain, bytes
#define BCF_LIST 2048u       // record offsets per window at most (then the window ends early)
#define BCF_MIN_SHARED 24u   // the six fixed words of the shared block

// error codes of a record (bits 8.. of its status word, like VCF_E_*)
#define BCF_E_SHARED 16    // l_shared below 24
#define BCF_E_TRUNC 17     // the record runs past the end of the batch
#define BCF_E_NSAMPLE 18   // n_sample differs from the header's sample count
#define BCF_E_NALT 19      // more than VCF_MAX_ALT alt alleles
#define BCF_E_FIELD 20     // a FORMAT field runs past l_indiv (or its key is no typed integer scalar)
#define BCF_E_TYPE 21      // an unknown type code
#define BCF_E_GT_TYPE 22   // GT is not of an integer type
#define BCF_E_NO_GT 23     // no GT among the FORMAT fields

#define BCF_HOP_RECORD 0
#define BCF_HOP_CARRY 1
#define BCF_HOP_BAD 2

// One hop of the chain: the record whose prefix (l_shared, l_indiv) was read at q, in a text of n bytes.
__host__ __device__ __forceinline__ int bcf_hop(unsigned l_shared, unsigned l_indiv, u64 q, u64 n, u64 *next)
{
    if (l_shared < BCF_MIN_SHARED) return BCF_HOP_BAD;
    const u64 e = q + 8ull + l_shared + l_indiv;
    if (e > n) return BCF_HOP_CARRY;
    *next = e;
    return BCF_HOP_RECORD;
}

__host__ __device__ __forceinline__ unsigned bcf_rd(const unsigned char *p, unsigned width)
{
    unsigned v = p[0];
    if (width > 1) v |= (unsigned)p[1] << 8;
    if (width > 2) v |= (unsigned)p[2] << 16 | (unsigned)p[3] << 24;
    return v;
}

// Bytes per value of a type code; -1: unknown.
__host__ __device__ __forceinline__ int bcf_type_size(unsigned type)
{
    switch (type) {
    case 0: return 0;
    case 1: return 1;
    case 2: return 2;
    case 3: return 4;
    case 5: return 4;
    case 7: return 1;
    default: return -1;
    }
}

// A typed integer scalar at p (below e): its value and the byte after it.  False: not one, or it runs past e.
__host__ __device__ inline bool bcf_int_scalar(const unsigned char *text, u64 *p, u64 e, unsigned *value)
{
    if (*p >= e) return false;
    const unsigned d = text[*p], type = d & 15u;
    if ((d >> 4) != 1u || type < 1u || type > 3u) return false;
    const unsigned w = (unsigned)bcf_type_size(type);
    if (*p + 1 + w > e) return false;
    *value = bcf_rd(text + *p + 1, w);
    *p += 1 + w;
    return true;
}

struct BcfGt {
    unsigned width;  // bytes per value (1, 2, 4); 0: an empty GT field (type 0 or length 0)
    unsigned len;    // values per sample
    unsigned at;     // offset of the first value
    unsigned n_alt;
};

// The record at o in text[0, n): its counts, then the walk over the FORMAT field headers up to the GT key.  0 or a
// BCF_E_* code.  Every read is below the record's end, and the record's end is at most n.
__host__ __device__ inline int bcf_find_gt(const unsigned char *text, u64 o, u64 n, unsigned n_samp, unsigned gt_key, BcfGt *g)
{
    if (o + 8 > n) return BCF_E_TRUNC;
    const unsigned l_shared = bcf_rd(text + o, 4), l_indiv = bcf_rd(text + o + 4, 4);
    if (l_shared < BCF_MIN_SHARED) return BCF_E_SHARED;
    const u64 e = o + 8ull + l_shared + l_indiv;
    if (e > n) return BCF_E_TRUNC;
    const unsigned n_allele = bcf_rd(text + o + 24, 4) >> 16;
    const unsigned fs = bcf_rd(text + o + 28, 4), n_fmt = fs >> 24;
    if ((fs & 0xFFFFFFu) != n_samp) return BCF_E_NSAMPLE;
    g->n_alt = n_allele > 2 ? n_allele - 1 : 1;  // (ALT `.` counts as one alt in read_vcf)
    if (g->n_alt > VCF_MAX_ALT) return BCF_E_NALT;
    u64 p = o + 8ull + l_shared;
    for (unsigned f = 0; f < n_fmt; ++f) {
        unsigned key;
        if (!bcf_int_scalar(text, &p, e, &key)) return BCF_E_FIELD;
        if (p >= e) return BCF_E_FIELD;
        const unsigned d = text[p++], type = d & 15u;
        unsigned len = d >> 4;
        if (len == 15u && !bcf_int_scalar(text, &p, e, &len)) return BCF_E_FIELD;
        const int size = bcf_type_size(type);
        if (size < 0) return BCF_E_TYPE;
        if (len > 0x7FFFFFFFu) return BCF_E_FIELD;
        const u64 bytes = (u64)n_samp * len * (unsigned)size;  // below 2^19 * 2^31 * 4
        if (bytes > e - p) return BCF_E_FIELD;
        if (key == gt_key) {
            if (type == 5u || type == 7u) return BCF_E_GT_TYPE;
            g->width = len ? (unsigned)size : 0u;
            g->len = len;
            g->at = (unsigned)p;
            return 0;
        }
        p += bytes;
    }
    return BCF_E_NO_GT;
}

__host__ __device__ __forceinline__ void bcf_count(unsigned *cnt, unsigned a)
{
#if defined(__HIP_DEVICE_COMPILE__)
    atomicAdd(&cnt[a], 1u);
#else
    ++cnt[a];
#endif
}

// One cell: g.len values of g.width bytes at p.  Counts every allele 0..n_alt in front of the end-of-vector sentinel
// into cnt; returns 1 = het, 2 = hom-alt, 0 = absent (ploidy below 2, a missing allele, or hom-ref).
__host__ __device__ inline int bcf_cell(const unsigned char *p, const BcfGt &g, unsigned *cnt)
{
    const unsigned miss_s = 1u << (8 * g.width - 1), eov = miss_s + 1;
    unsigned ploidy = 0, first = 0;
    bool missing = false, diff = false;
    for (unsigned k = 0; k < g.len; ++k) {
        const unsigned v = bcf_rd(p + (u64)k * g.width, g.width);
        if (v == eov) break;
        const bool miss = v == miss_s || (v >> 1) == 0;
        const unsigned a = (v >> 1) - 1;
        if (!miss && a <= g.n_alt) bcf_count(cnt, a);
        if (ploidy == 0) first = a;
        else diff |= miss || a != first;
        missing |= miss;
        ++ploidy;
    }
    if (ploidy < 2 || missing) return 0;
    return diff ? 1 : (first > 0 ? 2 : 0);
}

// ------------------------------------------------------------------------------------------------ the chain
// text[0, n) = carry, prefix, new bytes.  offs[i] = start of whole record i; misc[0] = their count, misc[2] = the offset
// behind the last of them (the carry is text[misc[2], n)).  A header of fewer than 8 bytes, or a record that runs past n,
// is carry.  A prefix with l_shared < 24 ends the walk: its offset is listed as a last record, misc[1] = its index (the
// host fails the batch at once; k_bcf_parse would fail it with BCF_E_SHARED as well), and nothing is carried.  offs holds
// n / 32 + 1 entries (a record is 32 bytes at least).  The walking lane reads a prefix as three aligned LDS words and
// shifts the two unaligned ones out of them.
__global__ __launch_bounds__(VCF_THREADS) void k_bcf_chain(const unsigned char *__restrict__ text, unsigned n,
                                                           unsigned *__restrict__ offs, unsigned *__restrict__ misc)
{
    __shared__ v4u s_win[BCF_WINDOW / 16 + 1];  // + one piece: the third word of a prefix at the window's end
    __shared__ unsigned s_list[BCF_LIST];
    __shared__ unsigned s_k, s_done;
    __shared__ u64 s_pos;
    const unsigned t = threadIdx.x;
    const unsigned *win = reinterpret_cast<const unsigned *>(s_win);
    u64 pos = 0;
    unsigned n_rec = 0, bad = 0xFFFFFFFFu;
    if (t == 0) s_win[BCF_WINDOW / 16] = v4u{0, 0, 0, 0};
    for (;;) {
        // the window: aligned 16 B pieces from the one that holds `pos`, up to the end of the text
        const u64 base = pos & ~15ull;
        const u64 lim = min((u64)n, base + BCF_WINDOW);  // bytes below lim are staged
        v4u r[BCF_WINDOW / 16 / VCF_THREADS];  // all of a lane's loads in flight at once: one round trip per window
#pragma unroll
        for (unsigned j = 0; j < BCF_WINDOW / 16 / VCF_THREADS; ++j) {
            const u64 a = base + 16ull * (t + j * VCF_THREADS);
            r[j] = a < lim ? *reinterpret_cast<const v4u *>(text + a) : v4u{0, 0, 0, 0};
        }
#pragma unroll
        for (unsigned j = 0; j < BCF_WINDOW / 16 / VCF_THREADS; ++j) s_win[t + j * VCF_THREADS] = r[j];
        __syncthreads();
        if (t == 0) {
            u64 q = pos;
            unsigned k = 0, done = 0;
            while (k < BCF_LIST) {
                if (q + 8 > n) {
                    done = 1;
                    break;
                }
                if (q + 8 > lim) break;  // the next prefix is not in this window
                const unsigned at = (unsigned)(q - base), sh = at & 3u;
                const unsigned w0 = win[at >> 2], w1 = win[(at >> 2) + 1], w2 = win[(at >> 2) + 2];
                const unsigned ls = __builtin_amdgcn_alignbyte(w1, w0, sh), li = __builtin_amdgcn_alignbyte(w2, w1, sh);
                u64 next = 0;
                const int hop = bcf_hop(ls, li, q, n, &next);
                if (hop == BCF_HOP_CARRY) {
                    done = 1;
                    break;
                }
                s_list[k++] = (unsigned)q;
                if (hop == BCF_HOP_BAD) {
                    bad = n_rec + k - 1;
                    q = n;
                    done = 1;
                    break;
                }
                q = next;
            }
            s_k = k;
            s_done = done;
            s_pos = q;
        }
        __syncthreads();
        const unsigned k = s_k, done = s_done;
        pos = s_pos;
        for (unsigned i = t; i < k; i += VCF_THREADS) offs[n_rec + i] = s_list[i];
        n_rec += k;
        __syncthreads();
        if (done) break;
    }
    if (t == 0) {
        misc[0] = n_rec;
        misc[2] = (unsigned)pos;
        if (bad != 0xFFFFFFFFu) misc[1] = bad;
    }
}

// ------------------------------------------------------------------------------------------------ one record
// Dynamic LDS: the record's presence row, ceil(n_samp / 32) words, as in k_vcf_parse; the same outputs.
__global__ __launch_bounds__(VCF_THREADS) void k_bcf_parse(const unsigned char *__restrict__ text, const unsigned *__restrict__ offs,
                                                           unsigned n, unsigned n_samp, unsigned row_words, unsigned row_bytes,
                                                           unsigned gt_key, unsigned char *__restrict__ rows,
                                                           double *__restrict__ af, unsigned *__restrict__ n_het,
                                                           unsigned *__restrict__ n_hom, unsigned *__restrict__ status,
                                                           unsigned *__restrict__ misc)
{
    extern __shared__ unsigned s_bits[];
    __shared__ unsigned s_cnt[VCF_MAX_ALT + 1];
    __shared__ unsigned s_red[4 * (VCF_THREADS / 64)];
    __shared__ BcfGt s_gt;
    __shared__ int s_err;

    const unsigned rec = blockIdx.x, t = threadIdx.x;
    if (t == 0) {
        BcfGt g = {0, 0, 0, 1};
        s_err = bcf_find_gt(text, offs[rec], n, n_samp, gt_key, &g);
        s_gt = g;
    }
    __syncthreads();
    const int err = s_err;
    if (err) {
        if (t == 0) {
            status[rec] = (unsigned)err << 8;
            af[rec] = 0.0;
            n_het[rec] = n_hom[rec] = 0;
            atomicMin(&misc[1], rec);
        }
        return;
    }
    const BcfGt g = s_gt;
    for (unsigned i = t; i <= g.n_alt; i += VCF_THREADS) s_cnt[i] = 0;
    for (unsigned i = t; i < row_words; i += VCF_THREADS) s_bits[i] = 0;
    __syncthreads();
    unsigned het = 0, hom = 0;
    if (g.width == 1 && g.len == 2) {
        // -- fast path: lane i of a pass takes the 16 bytes of samples 8 i .. 8 i + 7 and writes their row byte
        // per-thread counters of alleles 0..7 in 16-bit fields (a lane adds at most 16 per pass, and there are at most
        // 256 passes: 524,288 samples), LDS bins from allele 8 on
        u64 c_lo = 0, c_hi = 0;
        unsigned char *row = reinterpret_cast<unsigned char *>(s_bits);
        const unsigned sh = (g.at & 3u) * 8u, wsk = (g.at & 15u) >> 2;
        for (unsigned b = t; b < row_bytes; b += VCF_THREADS) {
            const unsigned p = g.at + 16u * b;  // 16 genotype bytes from p: assembled from the two aligned pieces around them
            const v4u lo = *reinterpret_cast<const v4u *>(text + (p & ~15u));
            const v4u hi = *reinterpret_cast<const v4u *>(text + (p & ~15u) + 16u);
            const unsigned x[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
            unsigned w[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                unsigned a = 0, bb = 0;
#pragma unroll
                for (int s = 0; s < 4; ++s) {  // (a select over constant indexes: x stays in registers)
                    a = wsk == (unsigned)s ? x[j + s] : a;
                    bb = wsk == (unsigned)s ? x[j + s + 1] : bb;
                }
                w[j] = sh ? (a >> sh) | (bb << (32u - sh)) : a;
            }
            const unsigned cells = min(8u, n_samp - 8u * b);
            unsigned byte = 0;
#pragma unroll
            for (unsigned k = 0; k < 8; ++k) {
                const unsigned pair = (w[k >> 1] >> (16u * (k & 1u))) & 0xFFFFu;
                const unsigned v0 = pair & 0xFFu, v1 = pair >> 8;
                const bool in = k < cells;
                const bool e0 = v0 == 0x81u, e1 = e0 || v1 == 0x81u;      // end of vector: ploidy 0 / below 2
                const bool m0 = v0 == 0x80u || (v0 >> 1) == 0, m1 = v1 == 0x80u || (v1 >> 1) == 0;
                const unsigned a0 = (v0 >> 1) - 1, a1 = (v1 >> 1) - 1;  // at most 62
                const bool k0 = in && !e0 && !m0 && a0 <= g.n_alt, k1 = in && !e1 && !m1 && a1 <= g.n_alt;
                const bool called = in && !e1 && !m0 && !m1;
                const bool h = called && a0 != a1, ha = called && a0 == a1 && a0 > 0;
                het += h;
                hom += ha;
                byte |= (unsigned)(h || ha) << (7u - k);
                const u64 i0 = k0 && a0 < 8u ? 1ull << (16u * (a0 & 3u)) : 0ull, i1 = k1 && a1 < 8u ? 1ull << (16u * (a1 & 3u)) : 0ull;
                c_lo += (a0 < 4u ? i0 : 0ull) + (a1 < 4u ? i1 : 0ull);
                c_hi += (a0 < 4u ? 0ull : i0) + (a1 < 4u ? 0ull : i1);
                if (k0 && a0 >= 8u) atomicAdd(&s_cnt[a0], 1u);
                if (k1 && a1 >= 8u) atomicAdd(&s_cnt[a1], 1u);
            }
            row[b] = (unsigned char)byte;
        }
#pragma unroll
        for (unsigned q = 0; q < 8; ++q) {
            const unsigned v = vcf_wave_sum((unsigned)((q < 4 ? c_lo : c_hi) >> (16u * (q & 3u))) & 0xFFFFu);
            if ((t & 63) == 0 && q <= g.n_alt && v) atomicAdd(&s_cnt[q], v);
        }
    } else if (g.width) {
        // -- general path: one sample per lane, any width and length
        const u64 cell = (u64)g.len * g.width;
        for (unsigned j = t; j < n_samp; j += VCF_THREADS) {
            const int r = bcf_cell(text + g.at + j * cell, g, s_cnt);
            het += r == 1;
            hom += r == 2;
            if (r) vcf_set_bit(s_bits, j);
        }
    }
    // -- counts -> AF, singleton flag; het / hom totals; the row (as in k_vcf_parse)
    __syncthreads();
    unsigned total = 0, mx = 0;
    for (unsigned i = t; i <= g.n_alt; i += VCF_THREADS) {
        const unsigned v = s_cnt[i];
        total += v;
        if (i) mx = max(mx, v);
    }
    total = vcf_wave_sum(total);
    mx = vcf_wave_max(mx);
    het = vcf_wave_sum(het);
    hom = vcf_wave_sum(hom);
    if ((t & 63) == 0) {
        s_red[t >> 6] = total;
        s_red[4 + (t >> 6)] = mx;
        s_red[8 + (t >> 6)] = het;
        s_red[12 + (t >> 6)] = hom;
    }
    __syncthreads();
    const unsigned char *row = reinterpret_cast<const unsigned char *>(s_bits);
    for (unsigned i = t; i < row_bytes; i += VCF_THREADS) rows[(u64)rec * row_bytes + i] = row[i];
    if (t == 0) {
        unsigned tt = 0, mm = 0, hh = 0, oo = 0;
        for (int w = 0; w < VCF_THREADS / 64; ++w) {
            tt += s_red[w];
            mm = max(mm, s_red[4 + w]);
            hh += s_red[8 + w];
            oo += s_red[12 + w];
        }
        af[rec] = tt ? (double)mm / (double)tt : 0.0;
        n_het[rec] = hh;
        n_hom[rec] = oo;
        status[rec] = (s_cnt[1] == 1 || s_cnt[0] == 1) ? VCF_F_SINGLETON : 0u;
    }
}
