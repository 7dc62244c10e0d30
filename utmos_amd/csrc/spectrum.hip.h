// Carrier counts: for a GIVEN list of samples, how many of them carry every variant, and the histogram of that count
// (utm_carrier_counts).
#pragma once
#include "common.hip.h"
#include "order.hip.h"
#include "swap.hip.h"

// ------------------------------------------------------------------------------------------------
// count[v] = the number of listed columns that carry variant v; hist[c] = the number of variants with count c that no
// `given` sample carries: the site-frequency spectrum of the list.
//
// One streaming pass over the n listed columns, shaped like k_capture_rank and k_swap_masks: a workgroup of four waves
// owns a 4 KiB tile of the variant axis, a wave one KiB of it (one global_load_dwordx4 wave instruction per column), a
// lane 16 bytes.  The lane keeps the count of its 128 variants as P bit planes of two words in registers (plane p = bit p
// of every variant's count), starting from zero, and walks the list in rounds of UTM_SPEC_B = 16 columns with the NEXT
// round's loads requested before this round's arithmetic.
//
// Counter: a round is one carry-save block (Harley-Seal).  The 16 words of a block are folded into the four low planes
// with 8 + 4 + 2 + 1 = 15 full adders (spec_csa: 5 logic operations on 64 bits each); what leaves plane 3 has weight 16
// and ripples through the planes 4 .. P-1 once per block.  Per column that is 15/16 adders + (P - 4)/8 operations,
// whatever P is -- rippling every column through all planes would cost 2 P operations (24 at n = 2,504 against about 6).
// The planes stay plain binary digits after every block, so a list that ends inside a block just feeds zero words.
// P is one of 4, 8, 12, 16, 20 (n < 16, 256, 4,096, 65,536, 2^20): the carry out of the top plane is always 0.
//
// After the last column: keep = the word's mask (uncov of k_swap_masks over the `given` columns, or the valid bits).
// Bins 0 .. 7 are popcounts of plane combinations under keep & ~(plane 3 | ... | plane P-1) -- under a 1/c spectrum, and
// more so beyond a `given` panel, that is where the variants are, and one atomic per variant on those few bins would
// serialise.  They are summed per wave (DPP) and meet in LDS.  Only the variants with a count of 8 or more are decoded
// bit by bit (ctz over keep & the OR of the higher planes) and added to a histogram in LDS (n + 1 <= UTM_SPEC_LDS_BINS
// bins of 32 bits: a tile has 32,768 variants) or, where that does not fit, straight to the global bins.  The workgroup
// flushes with one 64-bit global atomic per non-zero bin.  Integer sums: the order of the atomics cannot matter.
//
// COUNTS: one int32 per variant as well.  The host fills the buffer (0 without a mask, -1 with one) and the kernel
// stores only what differs: the non-zero counts, or the counts of the variants the mask keeps.  4-byte vector stores,
// 64 entries per word of the column, so no store can leave the buffer.
// ------------------------------------------------------------------------------------------------
#define UTM_SPEC_TILE_WORDS UTM_ORDER_TILE_WORDS  // a workgroup of four waves: 4 KiB of the variant axis
#define UTM_SPEC_B 16                             // columns per carry-save block = per round of loads
#define UTM_SPEC_LOW 4                            // planes a block folds into: log2(UTM_SPEC_B)
#define UTM_SPEC_POP_PLANES 3                     // bins below 2^3 are popcounts of plane combinations
#define UTM_SPEC_POP_BINS (1 << UTM_SPEC_POP_PLANES)
#define UTM_SPEC_LDS_BINS 4096                    // bins the LDS form holds (16 KiB)
#define UTM_SPEC_MAX_N ((1u << 20) - 1)           // 20 planes
static_assert(UTM_SPEC_B == UTM_ORDER_U, "a round of loads is one carry-save block");

// Full adder on 64 lanes of bits: a + b + c = 2 * h + l.
UTM_HD void spec_csa(u64 a, u64 b, u64 c, u64 &h, u64 &l)
{
    const u64 u = a ^ b;
    h = (a & b) | (u & c);
    l = u ^ c;
}

// One word of each of UTM_SPEC_B columns into the word's planes: the whole arithmetic of a block, shared with the CPU
// build (utm_carrier_counts_host).  Words past the end of the list are zero.
template <int P>
UTM_HD void spectrum_block(const u64 (&w)[UTM_SPEC_B], u64 (&pl)[P])
{
    static_assert(P >= UTM_SPEC_LOW, "a block folds into four planes");
    u64 t2[8], t4[4], t8[2], c, l = pl[0];
#pragma unroll
    for (int k = 0; k < 8; ++k) spec_csa(l, w[2 * k], w[2 * k + 1], t2[k], l);
    pl[0] = l;
    l = pl[1];
#pragma unroll
    for (int k = 0; k < 4; ++k) spec_csa(l, t2[2 * k], t2[2 * k + 1], t4[k], l);
    pl[1] = l;
    l = pl[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) spec_csa(l, t4[2 * k], t4[2 * k + 1], t8[k], l);
    pl[2] = l;
    spec_csa(pl[3], t8[0], t8[1], c, l);
    pl[3] = l;
#pragma unroll
    for (int p = UTM_SPEC_LOW; p < P; ++p) {  // (weight 16: once per block)
        const u64 t = pl[p] & c;
        pl[p] ^= c;
        c = t;
    }
}

// A finished word: low[b] += the variants of `keep` with a count of b < UTM_SPEC_POP_BINS; returns the kept variants
// with a higher count, and in `any` the variants with a count above 0.
template <int P>
UTM_HD u64 spectrum_low(const u64 (&pl)[P], u64 keep, unsigned (&low)[UTM_SPEC_POP_BINS], u64 &any)
{
    u64 hi = 0;
#pragma unroll
    for (int p = UTM_SPEC_POP_PLANES; p < P; ++p) hi |= pl[p];
    const u64 z = keep & ~hi;
#pragma unroll
    for (int b = 0; b < UTM_SPEC_POP_BINS; ++b) {
        u64 m = z;
#pragma unroll
        for (int p = 0; p < UTM_SPEC_POP_PLANES; ++p) m &= (b >> p & 1) ? pl[p] : ~pl[p];
        low[b] += (unsigned)__builtin_popcountll(m);
    }
    any = hi | pl[0] | pl[1] | pl[2];
    return keep & hi;
}

// The count of the variant at `bit` of a finished word.
template <int P>
UTM_HD unsigned spectrum_count(const u64 (&pl)[P], int bit)
{
    unsigned c = 0;
#pragma unroll
    for (int p = 0; p < P; ++p) c |= (unsigned)(pl[p] >> bit & 1u) << p;
    return c;
}

// The entries of count64[0..63] (the word's first variant onwards) that differ from what the buffer was filled with:
// without a mask (filled with 0) the non-zero counts, with one (filled with -1) the counts of the kept variants.
UTM_HD u64 spectrum_store_bits(u64 keep, u64 any, bool masked) { return masked ? keep : keep & any; }

// A finished word of a lane: popcounted bins into low[], the rest decoded into the LDS or the global bins, counts stored.
template <int P, bool COUNTS>
__device__ __forceinline__ void spectrum_finish(const u64 (&pl)[P], u64 keep, bool masked, unsigned (&low)[UTM_SPEC_POP_BINS],
                                                unsigned *lds_bins, u64 *hist, int32_t *count64)
{
    u64 any;
    const u64 rest = spectrum_low<P>(pl, keep, low, any);
    u64 todo = COUNTS ? spectrum_store_bits(keep, any, masked) : rest;  // (rest is a subset of the stored bits)
    while (todo) {
        const int bit = __builtin_ctzll(todo);
        todo &= todo - 1;
        const unsigned c = spectrum_count<P>(pl, bit);
        if (COUNTS) count64[bit] = (int32_t)c;
        if (c >= UTM_SPEC_POP_BINS) {
            if (lds_bins) atomicAdd(&lds_bins[c], 1u);
            else atomicAdd(&hist[c], (u64)1);
        }
    }
}

// hist: n + 1 bins, zeroed before the first launch.  mask: wp words (uncov of k_swap_masks), or nullptr = the valid bits.
// use_lds: the decoded variants meet in LDS (n + 1 <= UTM_SPEC_LDS_BINS), else they go to the global bins one by one.
// count: 64 * wp entries filled with mask ? -1 : 0 (COUNTS), else unused.
template <int P, bool NT, bool COUNTS>
__global__ __launch_bounds__(256) void k_carrier_counts(const u64 *__restrict__ cols, u64 wp, u64 n_var, const unsigned *__restrict__ list, unsigned n,
                                                        const u64 *__restrict__ mask, int use_lds, u64 *__restrict__ hist, int32_t *__restrict__ count)
{
    constexpr int U = UTM_SPEC_B;
    __shared__ unsigned bins[UTM_SPEC_LDS_BINS];
    __shared__ unsigned low_sum[UTM_SPEC_POP_BINS];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const u64 w0 = (u64)blockIdx.x * UTM_SPEC_TILE_WORDS + (u64)wave * UTM_STEP_WORDS;
    // wp is a multiple of UTM_STEP_WORDS: a wave's KiB lies inside the column or past its end as a whole.  A wave past
    // it (the column's last tile) loads and counts nothing, but keeps the barriers.
    const bool own = w0 < wp;
    const unsigned n_bins = use_lds ? n + 1 : 0;
    for (unsigned b = threadIdx.x; b < n_bins; b += 256) bins[b] = 0;
    if (threadIdx.x < UTM_SPEC_POP_BINS) low_sum[threadIdx.x] = 0;
    __syncthreads();
    if (own) {
        const v2q *base = reinterpret_cast<const v2q *>(cols + w0) + lane;
        const u64 stride = wp / 2;  // a column, in 16-byte units
#define UTM_SPEC_LOAD(DST, I0)                                                                           \
    _Pragma("unroll") for (int u = 0; u < U; ++u) if ((I0) + u < n)                                      \
    {                                                                                                    \
        const v2q *p_ = base + (u64)list[(I0) + u] * stride;                                             \
        DST[u] = NT ? __builtin_nontemporal_load(p_) : *p_;                                              \
    }
        v2q x[U], y[U];
#pragma unroll
        for (int u = 0; u < U; ++u) x[u] = y[u] = v2q{0, 0};
        UTM_SPEC_LOAD(x, 0u)
        u64 a[P], b[P];
#pragma unroll
        for (int p = 0; p < P; ++p) a[p] = b[p] = 0;
        for (unsigned i = 0; i < n; i += U) {
            if (i + U < n) { UTM_SPEC_LOAD(y, i + U) }
            u64 wa[U], wb[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const bool in = i + u < n;  // (uniform; a slot past the list still holds an earlier round's word)
                wa[u] = in ? x[u].x : 0ull;
                wb[u] = in ? x[u].y : 0ull;
            }
            spectrum_block<P>(wa, a);
            spectrum_block<P>(wb, b);
#pragma unroll
            for (int u = 0; u < U; ++u) x[u] = y[u];
        }
#undef UTM_SPEC_LOAD
        const u64 w = w0 + 2 * (u64)lane;
        v2q keep = v2q{swap_valid(w, n_var), swap_valid(w + 1, n_var)};
        if (mask) keep = reinterpret_cast<const v2q *>(mask + w0)[lane];
        unsigned low[UTM_SPEC_POP_BINS];
#pragma unroll
        for (int q = 0; q < UTM_SPEC_POP_BINS; ++q) low[q] = 0;
        int32_t *mine = COUNTS ? count + w * 64 : nullptr;  // the lane's 128 variants
        spectrum_finish<P, COUNTS>(a, keep.x, mask != nullptr, low, use_lds ? bins : nullptr, hist, mine);
        spectrum_finish<P, COUNTS>(b, keep.y, mask != nullptr, low, use_lds ? bins : nullptr, hist, COUNTS ? mine + 64 : nullptr);
#pragma unroll
        for (int q = 0; q < UTM_SPEC_POP_BINS; ++q) {
            const unsigned s = wave_sum_u32(low[q]);
            if (lane == 0 && s) atomicAdd(&low_sum[q], s);
        }
    }
    __syncthreads();
    // bins below UTM_SPEC_POP_BINS come from low_sum alone: the decode never adds to them
    if (threadIdx.x < UTM_SPEC_POP_BINS && threadIdx.x <= n && low_sum[threadIdx.x])
        __hip_atomic_fetch_add(&hist[threadIdx.x], (u64)low_sum[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (unsigned q = UTM_SPEC_POP_BINS + threadIdx.x; q < n_bins; q += 256)
        if (bins[q]) __hip_atomic_fetch_add(&hist[q], (u64)bins[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
