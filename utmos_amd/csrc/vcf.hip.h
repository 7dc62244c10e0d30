// VCF genotype parsing on the GPU: text of whole records (header removed, newline-terminated) -> the reference's packed
// rows, AF and het / hom-alt counts (utmos/convert.py:43-88 via scikit-allel; the CPU restatement is utmos_amd/vcfio.py).
//
//   k_vcf_nl_count   16 B per lane: '\n' count per 4 KiB block
//   k_vcf_nl_scan    one workgroup: exclusive scan of the block counts, record count
//   k_vcf_nl_write   the same 16 B per lane again: the offset of every '\n' (= the end of record i; record i starts
//                    one byte after the end of record i-1, record 0 at offset 0)
//   k_vcf_parse      one 256-thread workgroup per record: the first nine tabs, n_alt, GT's index in FORMAT, then the
//                    sample cells -- a fixed-offset fast path for `GT` + `a|b` cells, a tab-scan path for the rest
//
// Offsets are 32-bit: a batch holds less than 4 GiB (the host side enforces it).  The text buffer is readable 16 B past
// its end, so a lane's 16-byte load never leaves it.
#pragma once
#include "common.hip.h"

#define VCF_THREADS 256
#define VCF_BLOCK_BYTES (VCF_THREADS * 16)  // one 16 B load per lane
#define VCF_MAX_ALT 4096                    // LDS allele counters per record; more alt alleles -> VCF_E_NALT

// per-record status word: bit 0 singleton, bit 1 skipped (`##` line or empty line), bits 8.. error code
#define VCF_F_SINGLETON 1u
#define VCF_F_SKIP 2u
#define VCF_E_COLUMNS 1    // fewer than ten columns
#define VCF_E_CELLS 2      // sample cells != samples in the header
#define VCF_E_NO_GT 3      // no GT key in FORMAT, or a cell without the GT subfield
#define VCF_E_ALLELE 4     // an allele token that is neither `.` nor an unsigned decimal
#define VCF_E_NALT 5       // more than VCF_MAX_ALT alt alleles
#define VCF_E_HEADER 6     // a #CHROM line among the records
#define VCF_E_RANGE 7      // an allele above 10^18

// Bit i of the result = byte i of v equals c, for the bytes whose offset cb + i lies in [lo, hi).
__device__ __forceinline__ unsigned vcf_match16(v4u v, unsigned c, unsigned cb, unsigned lo, unsigned hi)
{
    const unsigned pat = c * 0x01010101u;
    unsigned m = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const unsigned x = v[k] ^ pat;
        const unsigned z = ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);  // 0x80 in every zero byte, exactly
        m |= (((z >> 7) & 1u) | ((z >> 14) & 2u) | ((z >> 21) & 4u) | ((z >> 28) & 8u)) << (4 * k);
    }
    const unsigned a = lo > cb ? min(lo - cb, 16u) : 0u;
    const unsigned b = hi > cb ? min(hi - cb, 16u) : 0u;
    return m & ((1u << b) - 1u) & ~((1u << a) - 1u);
}

// Exclusive prefix sum over a 256-thread workgroup; *total = the sum.  Ends with the workgroup synchronised.
__device__ __forceinline__ unsigned vcf_scan(unsigned v, unsigned *s_wave, unsigned *total)
{
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    unsigned x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned y = __shfl_up(x, d);
        if (lane >= d) x += y;
    }
    if (lane == 63) s_wave[wid] = x;
    __syncthreads();
    unsigned off = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < VCF_THREADS / 64; ++w) {
        const unsigned t = s_wave[w];
        off += w < wid ? t : 0u;
        tot += t;
    }
    __syncthreads();
    *total = tot;
    return off + x - v;
}

__device__ __forceinline__ unsigned vcf_wave_sum(unsigned x)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) x += __shfl_xor(x, d);
    return x;
}
__device__ __forceinline__ unsigned vcf_wave_max(unsigned x)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) x = max(x, (unsigned)__shfl_xor(x, d));
    return x;
}

// ------------------------------------------------------------------------------------------------ record ends
__global__ __launch_bounds__(VCF_THREADS) void k_vcf_nl_count(const unsigned char *__restrict__ text, unsigned n,
                                                              unsigned *__restrict__ blk_cnt)
{
    __shared__ unsigned s_wave[VCF_THREADS / 64];
    const unsigned cb = blockIdx.x * VCF_BLOCK_BYTES + threadIdx.x * 16;
    unsigned c = 0;
    if (cb < n) c = __popc(vcf_match16(*reinterpret_cast<const v4u *>(text + cb), '\n', cb, 0, n));
    c = vcf_wave_sum(c);
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) blk_cnt[blockIdx.x] = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
}

// blk_cnt -> exclusive offsets in place; misc[0] = records, misc[1] = first failing record (none: 0xFFFFFFFF)
__global__ __launch_bounds__(VCF_THREADS) void k_vcf_nl_scan(unsigned *__restrict__ blk_cnt, unsigned n_blk,
                                                             unsigned *__restrict__ misc)
{
    __shared__ unsigned s_wave[VCF_THREADS / 64];
    unsigned carry = 0;
    for (unsigned base = 0; base < n_blk; base += VCF_THREADS) {
        const unsigned i = base + threadIdx.x;
        const unsigned v = i < n_blk ? blk_cnt[i] : 0u;
        unsigned tot;
        const unsigned off = vcf_scan(v, s_wave, &tot);
        if (i < n_blk) blk_cnt[i] = carry + off;
        carry += tot;
    }
    if (threadIdx.x == 0) {
        misc[0] = carry;
        misc[1] = 0xFFFFFFFFu;
    }
}

__global__ __launch_bounds__(VCF_THREADS) void k_vcf_nl_write(const unsigned char *__restrict__ text, unsigned n,
                                                              const unsigned *__restrict__ blk_off, unsigned *__restrict__ nl)
{
    __shared__ unsigned s_wave[VCF_THREADS / 64];
    const unsigned cb = blockIdx.x * VCF_BLOCK_BYTES + threadIdx.x * 16;
    unsigned m = 0;
    if (cb < n) m = vcf_match16(*reinterpret_cast<const v4u *>(text + cb), '\n', cb, 0, n);
    unsigned tot;
    unsigned k = blk_off[blockIdx.x] + vcf_scan(__popc(m), s_wave, &tot);
    for (; m; m &= m - 1) nl[k++] = cb + __ffs(m) - 1;
}

// ------------------------------------------------------------------------------------------------ one record
// One GT subfield starting at p (its cell ends at '\t' or e).  Counts alleles 0..n_alt into s_cnt; *pres / *het / *hom
// follow vcfio._cells_slow: called = ploidy >= 2 and no `.`; het = called and some allele differs from the first;
// hom-alt = called, all equal, first > 0.  Returns 0 or a VCF_E_* code.
__device__ int vcf_cell(const unsigned char *__restrict__ text, unsigned p, unsigned e, int gi, unsigned n_alt,
                        unsigned *s_cnt, unsigned *het, unsigned *hom)
{
    for (int k = 0; k < gi; ++k) {
        while (p < e && text[p] != ':' && text[p] != '\t') ++p;
        if (p >= e || text[p] != ':') return VCF_E_NO_GT;
        ++p;
    }
    unsigned nal = 0;
    bool missing = false, diff = false;
    u64 first = 0;
    for (;;) {
        unsigned c = p < e ? text[p] : '\t';
        u64 a = 0;
        bool miss = false;
        if (c == '.') {
            miss = true;
            ++p;
        } else if (c - '0' < 10u) {
            int digits = 0;
            while (c - '0' < 10u) {
                a = a * 10 + (c - '0');
                digits += (a != 0);
                if (digits > 18) return VCF_E_RANGE;
                ++p;
                c = p < e ? text[p] : '\t';
            }
        } else {
            return VCF_E_ALLELE;  // empty token or a foreign character
        }
        if (!miss && a <= n_alt) atomicAdd(&s_cnt[a], 1u);
        if (nal == 0) first = a;
        else diff |= (miss || a != first);
        missing |= miss;
        ++nal;
        c = p < e ? text[p] : '\t';
        if (c == '/' || c == '|') {
            ++p;
            continue;
        }
        if (c == ':' || c == '\t') break;
        return VCF_E_ALLELE;
    }
    const bool called = nal > 1 && !missing;
    *het += called && diff;
    *hom += called && !diff && first > 0;
    return 0;
}

// Presence bit of sample j in the LDS row: numpy.packbits order inside little-endian 32-bit words.
__device__ __forceinline__ void vcf_set_bit(unsigned *s_bits, unsigned j)
{
    atomicOr(&s_bits[j >> 5], 1u << ((j & 24u) + 7u - (j & 7u)));
}

// Dynamic LDS: the record's presence row, ceil(n_samp / 32) words.  rows[rec * row_bytes + b] (packed: one contiguous
// copy to the host); status / af / het / hom
// one entry per record; misc[1] = lowest failing record (atomicMin).
__global__ __launch_bounds__(VCF_THREADS) void k_vcf_parse(const unsigned char *__restrict__ text, const unsigned *__restrict__ nl,
                                                           unsigned n_samp, unsigned row_words, unsigned row_bytes,
                                                           unsigned char *__restrict__ rows,
                                                           double *__restrict__ af, unsigned *__restrict__ n_het,
                                                           unsigned *__restrict__ n_hom, unsigned *__restrict__ status,
                                                           unsigned *__restrict__ misc)
{
    extern __shared__ unsigned s_bits[];
    __shared__ unsigned s_cnt[VCF_MAX_ALT + 1];
    __shared__ v4u s_win[VCF_THREADS + 1];
    __shared__ unsigned s_wave[VCF_THREADS / 64];
    __shared__ unsigned s_tabs[9];
    __shared__ unsigned s_red[4 * (VCF_THREADS / 64)];
    __shared__ int s_gi, s_fmt_gt, s_err;

    const unsigned rec = blockIdx.x, t = threadIdx.x;
    const unsigned s = rec ? nl[rec - 1] + 1 : 0u;
    unsigned e = nl[rec];
    while (e > s && text[e - 1] == '\r') --e;  // CRLF (read_vcf: raw.rstrip(b"\r\n"))
    unsigned flags = 0;
    int err = 0;
    if (e == s || (text[s] == '#' && e - s >= 2 && text[s + 1] == '#')) flags = VCF_F_SKIP;  // uniform: every thread reads the same bytes
    else if (e - s >= 6 && text[s] == '#' && text[s + 1] == 'C' && text[s + 2] == 'H' && text[s + 3] == 'R' &&
             text[s + 4] == 'O' && text[s + 5] == 'M')
        err = VCF_E_HEADER;
    if (flags || err) goto done;

    {
        // -- the first nine tabs, 4 KiB per pass (INFO may be long)
        unsigned found = 0;
        for (unsigned wb = s & ~15u; wb < e && found < 9; wb += VCF_BLOCK_BYTES) {
            const unsigned cb = wb + t * 16;
            unsigned m = cb < e ? vcf_match16(*reinterpret_cast<const v4u *>(text + cb), '\t', cb, s, e) : 0u;
            unsigned tot;
            unsigned k = found + vcf_scan(__popc(m), s_wave, &tot);
            for (; m && k < 9; m &= m - 1) s_tabs[k++] = cb + __ffs(m) - 1;
            found += tot;
        }
        if (t == 0) s_err = 0;
        __syncthreads();
        if (found < 9) {
            err = VCF_E_COLUMNS;
            goto done;
        }
        // -- n_alt = commas in ALT + 1; GT's index among the FORMAT keys
        unsigned commas = 0;
        for (unsigned i = s_tabs[3] + 1 + t; i < s_tabs[4]; i += VCF_THREADS) commas += text[i] == ',';
        unsigned n_alt;
        vcf_scan(commas, s_wave, &n_alt);
        n_alt += 1;
        if (n_alt > VCF_MAX_ALT) {
            err = VCF_E_NALT;
            goto done;
        }
        if (t == 0) {
            const unsigned f0 = s_tabs[7] + 1, f1 = s_tabs[8];
            int gi = -1, key = 0;
            for (unsigned p = f0; p <= f1 && gi < 0; ++key) {
                unsigned q = p;
                while (q < f1 && text[q] != ':') ++q;
                if (q - p == 2 && text[p] == 'G' && text[p + 1] == 'T') gi = key;
                p = q + 1;
            }
            s_gi = gi;
            s_fmt_gt = f1 - f0 == 2 && gi == 0;
        }
        for (unsigned i = t; i <= n_alt; i += VCF_THREADS) s_cnt[i] = 0;
        for (unsigned i = t; i < row_words; i += VCF_THREADS) s_bits[i] = 0;
        __syncthreads();
        const int gi = s_gi;
        const unsigned r0 = s_tabs[8] + 1;
        unsigned het = 0, hom = 0;

        // -- fast path: FORMAT is GT and the sample columns are n_samp cells `a|b` / `a/b` of width 3 (vcfio._cells_fast)
        bool fast = s_fmt_gt && (u64)(e - r0) == 4ull * n_samp - 1;
        if (fast) {
            unsigned c[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
            bool bad = false;
            for (unsigned wb = r0 & ~15u; wb < e; wb += VCF_BLOCK_BYTES) {
                const unsigned cb = wb + t * 16;
                s_win[t] = cb < e ? *reinterpret_cast<const v4u *>(text + cb) : v4u{0, 0, 0, 0};
                if (t == 0) {
                    const unsigned cx = wb + VCF_BLOCK_BYTES;
                    s_win[VCF_THREADS] = cx < e ? *reinterpret_cast<const v4u *>(text + cx) : v4u{0, 0, 0, 0};
                }
                __syncthreads();
                const unsigned char *wbytes = reinterpret_cast<const unsigned char *>(s_win);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const unsigned p = cb + ((r0 - cb) & 3u) + 4u * q;  // cells start at r0 + 4j
                    if (p < r0 || p >= e) continue;
                    const unsigned j = (p - r0) >> 2;
                    const unsigned o = p - wb;
                    const unsigned a0 = wbytes[o] - '0', sep = wbytes[o + 1], a1 = wbytes[o + 2] - '0', tb = wbytes[o + 3];
                    const bool d0 = a0 < 10u, d1 = a1 < 10u;
                    bad |= !(sep == '|' || sep == '/') || !(d0 || a0 == (unsigned)('.' - '0')) ||
                           !(d1 || a1 == (unsigned)('.' - '0')) || !(p + 3 == e || tb == '\t');
                    const bool called = d0 && d1;
                    const bool h = called && a0 != a1, ha = called && a0 == a1 && a0 > 0;
                    het += h;
                    hom += ha;
                    if (h || ha) vcf_set_bit(s_bits, j);
#pragma unroll
                    for (unsigned k = 0; k < 10; ++k) c[k] += (a0 == k) + (a1 == k);
                }
                __syncthreads();
            }
            fast = !__syncthreads_or(bad);
            if (fast) {
#pragma unroll
                for (unsigned k = 0; k < 10; ++k) {
                    const unsigned v = vcf_wave_sum(c[k]);
                    if ((t & 63) == 0 && k <= n_alt && v) atomicAdd(&s_cnt[k], v);
                }
            } else {  // not of that shape after all: start over on the general path
                het = hom = 0;
                for (unsigned i = t; i < row_words; i += VCF_THREADS) s_bits[i] = 0;
            }
        }
        // -- general path: a workgroup-wide tab scan numbers the cells; the thread that owns a cell's leading tab parses it
        if (!fast) {
            if (gi < 0) {
                err = VCF_E_NO_GT;
                goto done;
            }
            unsigned cells = 1;  // cell 0 starts at r0
            if (t == 0) {
                const int ce = vcf_cell(text, r0, e, gi, n_alt, s_cnt, &het, &hom);
                if (ce) atomicMax(&s_err, ce);
                else if (het + hom) vcf_set_bit(s_bits, 0);
            }
            for (unsigned wb = r0 & ~15u; wb < e; wb += VCF_BLOCK_BYTES) {
                const unsigned cb = wb + t * 16;
                unsigned m = cb < e ? vcf_match16(*reinterpret_cast<const v4u *>(text + cb), '\t', cb, r0, e) : 0u;
                unsigned tot;
                unsigned j = cells + vcf_scan(__popc(m), s_wave, &tot);
                for (; m; m &= m - 1, ++j) {
                    if (j >= n_samp) break;  // too many cells: reported below
                    const unsigned before = het + hom;
                    const int ce = vcf_cell(text, cb + __ffs(m), e, gi, n_alt, s_cnt, &het, &hom);
                    if (ce) atomicMax(&s_err, ce);
                    else if (het + hom != before) vcf_set_bit(s_bits, j);
                }
                cells += tot;
            }
            __syncthreads();
            if (cells != n_samp) err = VCF_E_CELLS;
            else err = s_err;
            if (err) goto done;
        }

        // -- counts -> AF, singleton flag; het / hom totals; the row
        __syncthreads();
        unsigned total = 0, mx = 0;
        for (unsigned i = t; i <= n_alt; i += VCF_THREADS) {
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
        const unsigned char *row = reinterpret_cast<const unsigned char *>(s_bits);  // little-endian words = packbits bytes
        for (unsigned i = t; i < row_bytes; i += VCF_THREADS) rows[(u64)rec * row_bytes + i] = row[i];
        if (t == 0) {
            unsigned tt = 0, mm = 0, hh = 0, oo = 0;
            for (int w = 0; w < VCF_THREADS / 64; ++w) {
                tt += s_red[w];
                mm = max(mm, s_red[4 + w]);
                hh += s_red[8 + w];
                oo += s_red[12 + w];
            }
            af[rec] = tt ? (double)mm / (double)tt : 0.0;  // == (counts[1:] / total).max(): IEEE division is monotonic
            n_het[rec] = hh;
            n_hom[rec] = oo;
            status[rec] = (s_cnt[1] == 1 || s_cnt[0] == 1) ? VCF_F_SINGLETON : 0u;
        }
        return;
    }
done:
    if (t == 0) {
        status[rec] = flags | ((unsigned)err << 8);
        af[rec] = 0.0;
        n_het[rec] = n_hom[rec] = 0;
        if (err) atomicMin(&misc[1], rec);
    }
}
