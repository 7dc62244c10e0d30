// Variant filters: drop rows of the bit-packed, column-major matrix by a keep mask (utm_filter_variants).
#pragma once
#include "common.hip.h"

// ------------------------------------------------------------------------------------------------
// Dropping rows is a bit-level stream compaction: output bit prefix[w] + rank(b) = input bit 64 w + b for every set bit b
// of keep[w], for every column alike.  gfx950 has no extract-bits-by-mask instruction, so a word is compressed with the
// parallel-suffix method (Hacker's Delight 7-4): six move masks derived from the keep word, then six and/shift/xor rounds
// per data word.  The masks depend on the keep word only, and the same keep word serves every column: a lane owns two
// consecutive input words (the 16-byte load of the scoring kernels: a wave reads one KiB of ONE column per instruction),
// derives their masks once, keeps them in registers and walks a run of columns.
//
// A compressed word is a piece of popcount(keep[w]) bits at output bit offset prefix[w]: it straddles output words at
// every possible shift.  The pieces of a wave's KiB (at most 8,192 bits behind an offset below 64: 129 output words)
// are merged by 64-bit LDS atomic ORs -- a piece that is zero, most of a sparse matrix, costs none -- and read back word
// by word.  Words that lie wholly inside the wave's output range go out as plain coalesced stores; the first and the last
// one may be shared with the neighbouring waves and go out by 64-bit vector atomic OR into the zero-filled destination
// (zeros are not sent).  UTM_FILTER_U columns are in flight per round, each with an LDS image of its own, so that a round
// costs two barriers.  Lanes whose two keep words are zero load nothing; a tile that keeps nothing leaves at once.
// ------------------------------------------------------------------------------------------------
#define UTM_FILTER_TILE_WORDS (4 * UTM_STEP_WORDS)  // a workgroup of four waves: 4 KiB of the variant axis
#define UTM_FILTER_U 4                              // columns per round
#define UTM_FILTER_LDS_WORDS 132                    // 129 output words of a wave's KiB + the word a straddling piece may touch, rounded up
#define UTM_FILTER_SCAN_THREADS 1024
#define UTM_FILTER_SCAN_WPT 16                      // keep words per thread and round of k_filter_prefix

struct FilterMasks {
    u64 m;      // the keep word
    u64 mv[6];  // bits to move right by 1, 2, 4, 8, 16, 32
};

UTM_HD void filter_masks(u64 m, FilterMasks &f)
{
    f.m = m;
    u64 mk = ~m << 1;  // the zeros to the right of every bit are counted
    for (int i = 0; i < 6; ++i) {
        u64 mp = mk ^ (mk << 1);  // parallel suffix
        mp ^= mp << 2;
        mp ^= mp << 4;
        mp ^= mp << 8;
        mp ^= mp << 16;
        mp ^= mp << 32;
        const u64 mv = mp & m;
        f.mv[i] = mv;
        m = (m ^ mv) | (mv >> (1 << i));
        mk &= ~mp;
    }
}

// The bits of x under the keep word, packed towards bit 0.
UTM_HD u64 filter_compress(u64 x, const FilterMasks &f)
{
    x &= f.m;
    for (int i = 0; i < 6; ++i) {
        const u64 t = x & f.mv[i];
        x = (x ^ t) | (t >> (1 << i));
    }
    return x;
}

// A piece at bit offset `at` of a word array: what goes into word at >> 6 (lo) and into the word behind it (hi).
UTM_HD void filter_piece(u64 piece, u64 at, u64 &lo, u64 &hi)
{
    const unsigned s = (unsigned)(at & 63);
    lo = piece << s;
    hi = s ? piece >> (64 - s) : 0;
}

// prefix[w] = the set bits of keep[0, w), w = 0 .. n_words (the last entry is the kept count).  ONE workgroup: a thread
// sums UTM_FILTER_SCAN_WPT consecutive words, the workgroup scans the sums, a carry runs from round to round -- ten rounds
// for the 156,250 keep words of 10M variants, next to a pass over the whole matrix.
__global__ __launch_bounds__(UTM_FILTER_SCAN_THREADS) void k_filter_prefix(const u64 *__restrict__ keep, u64 n_words, u64 *__restrict__ prefix)
{
    constexpr int WPT = UTM_FILTER_SCAN_WPT, WAVES = UTM_FILTER_SCAN_THREADS / 64;
    __shared__ unsigned wave_total[WAVES];
    const unsigned tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    u64 carry = 0;
    for (u64 base = 0; base < n_words; base += (u64)UTM_FILTER_SCAN_THREADS * WPT) {  // (uniform)
        const u64 w0 = base + (u64)tid * WPT;
        unsigned pc[WPT], sum = 0;
#pragma unroll
        for (int k = 0; k < WPT; ++k) {
            pc[k] = w0 + k < n_words ? (unsigned)__popcll(keep[w0 + k]) : 0u;
            sum += pc[k];
        }
        const unsigned incl = wave_scan_incl_u32(sum);
        if (lane == 63) wave_total[wave] = incl;
        __syncthreads();
        unsigned before = 0, total = 0;
        for (unsigned j = 0; j < (unsigned)WAVES; ++j) {
            const unsigned t = wave_total[j];
            before += j < wave ? t : 0u;
            total += t;
        }
        u64 run = carry + before + (incl - sum);
#pragma unroll
        for (int k = 0; k < WPT; ++k)
            if (w0 + k < n_words) {
                prefix[w0 + k] = run;
                run += pc[k];
            }
        carry += total;
        __syncthreads();  // (wave_total is written again in the next round)
    }
    if (tid == 0) prefix[n_words] = carry;
}

// cols[c * wp + w] -> out[c * wp_out + ...] for the columns c = list[j] (list == nullptr: c = j), j in [blockIdx.y *
// cols_per_group, + cols_per_group) below n_cols, and the input tile blockIdx.x.  A column keeps its index; one that is not
// listed is neither read nor written (the destination's zero fill stands for it).  w_in = the words of keep[] (bits at or
// above n_var are clear), prefix[w_in + 1] from k_filter_prefix, `out` zero-filled.  Loads: only where a keep word is set,
// so below w_in <= wp.  Stores: word g of a column only for 64 g < prefix[w_in] <= 64 wp_out.
template <bool NT>
__global__ __launch_bounds__(256) void k_filter_compact(const u64 *__restrict__ cols, u64 wp, u64 w_in, const u64 *__restrict__ keep,
                                                        const u64 *__restrict__ prefix, u64 *__restrict__ out, u64 wp_out, unsigned n_cols,
                                                        unsigned cols_per_group, const unsigned *__restrict__ list)
{
    constexpr int U = UTM_FILTER_U;
    __shared__ u64 image[4][U][UTM_FILTER_LDS_WORDS];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const u64 w0 = (u64)blockIdx.x * UTM_FILTER_TILE_WORDS + (u64)wave * UTM_STEP_WORDS;
    const u64 wl = w0 + 2 * (u64)lane;  // the lane's two input words
    const u64 k0 = wl < w_in ? keep[wl] : 0, k1 = wl + 1 < w_in ? keep[wl + 1] : 0;
    const bool mine = (k0 | k1) != 0;
    if (!__syncthreads_or(mine)) return;  // the tile keeps nothing
    // the wave's output range, in bits: [first, end), and the output word its LDS image starts at
    const u64 first = prefix[w0 < w_in ? w0 : w_in], end = prefix[w0 + UTM_STEP_WORDS < w_in ? w0 + UTM_STEP_WORDS : w_in];
    const u64 word0 = first >> 6;
    const unsigned first_rel = (unsigned)(first & 63), end_rel = (unsigned)(end - (word0 << 6));  // (at most 63 + 8,192)
    const unsigned n_out = end > first ? (end_rel + 63) >> 6 : 0;                                 // (at most 129)
    const unsigned at0 = mine ? (unsigned)(prefix[wl] - (word0 << 6)) : 0, at1 = at0 + (unsigned)__popcll(k0);
    FilterMasks f0, f1;
    filter_masks(k0, f0);
    filter_masks(k1, f1);
    for (unsigned k = lane; k < UTM_FILTER_LDS_WORDS; k += 64)
#pragma unroll
        for (int u = 0; u < U; ++u) image[wave][u][k] = 0;
    __syncthreads();
    const unsigned c_begin = blockIdx.y * cols_per_group, c_end = c_begin + cols_per_group < n_cols ? c_begin + cols_per_group : n_cols;
    const v2q *src = reinterpret_cast<const v2q *>(cols + wl);
    const u64 stride = wp / 2;  // a column, in 16-byte units
    for (unsigned c = c_begin; c < c_end; c += U) {  // (uniform over the workgroup)
        v2q x[U];
        unsigned col[U];  // (uniform: the columns of this round)
#pragma unroll
        for (int u = 0; u < U; ++u) {
            col[u] = c + u < c_end ? (list ? list[c + u] : c + u) : 0u;
            x[u] = v2q{0, 0};
            if (mine && c + u < c_end) x[u] = NT ? __builtin_nontemporal_load(src + (u64)col[u] * stride) : src[(u64)col[u] * stride];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            u64 lo, hi;
            const u64 a = filter_compress(x[u].x, f0), b = filter_compress(x[u].y, f1);
            if (a) {
                filter_piece(a, at0, lo, hi);
                atomicOr(&image[wave][u][at0 >> 6], lo);
                if (hi) atomicOr(&image[wave][u][(at0 >> 6) + 1], hi);
            }
            if (b) {
                filter_piece(b, at1, lo, hi);
                atomicOr(&image[wave][u][at1 >> 6], lo);
                if (hi) atomicOr(&image[wave][u][(at1 >> 6) + 1], hi);
            }
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (c + u >= c_end) break;  // (uniform)
            u64 *dst = out + (u64)col[u] * wp_out + word0;
            for (unsigned k = lane; k < n_out; k += 64) {
                const u64 v = image[wave][u][k];
                image[wave][u][k] = 0;
                const bool whole = k * 64 >= first_rel && (k + 1) * 64 <= end_rel;  // no other wave writes into this word
                if (whole) dst[k] = v;
                else if (v) atomicOr(dst + k, v);
            }
        }
        __syncthreads();  // (the images are zero again before the next round's pieces arrive)
    }
}

// ------------------------------------------------------------------------------------------------
// The integer loop's working view (host_compact.hip.h): the keep mask of a compaction is what is still uncovered, and
// while a view is scored the chunk's own covered mask is brought up to date from the result rows.
// ------------------------------------------------------------------------------------------------
// keep[i] = ~covered[i] for the n_words words that hold variants, the bits at or above n_var clear.
__global__ __launch_bounds__(256) void k_compact_keep(const u64 *__restrict__ covered, u64 n_words, u64 n_var, u64 *__restrict__ keep)
{
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < n_words; i += (u64)gridDim.x * 256) {
        u64 k = ~covered[i];
        if (i == n_words - 1 && (n_var & 63)) k &= (1ull << (n_var & 63)) - 1;
        keep[i] = k;
    }
}

// The same from a working view: what neither the view's mask nor the pending winner's column in the view covers (the
// view's mask lacks the pending winner until the next scoring launch applies it).  An eligible context is the only
// shard, so the pending column, if there is one, is a column of `cols`.
__global__ __launch_bounds__(256) void k_view_keep(const u64 *__restrict__ covered, const u64 *__restrict__ cols, u64 wp, const Pending pend,
                                                   const IterState *__restrict__ st, u64 n_words, u64 n_var, u64 *__restrict__ keep)
{
    const u64 *wcol = pending_column(st, cols, wp, pend);
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < n_words; i += (u64)gridDim.x * 256) {
        u64 k = ~(covered[i] | (wcol ? wcol[i] : 0ull));
        if (i == n_words - 1 && (n_var & 63)) k &= (1ull << (n_var & 63)) - 1;
        keep[i] = k;
    }
}

// covered |= the columns of the winners of result rows [r0, r1) (global sample indices; this context holds them all):
// one pass over covered, every thread ORs its word of every winner.
__global__ __launch_bounds__(256) void k_or_rows(u64 *__restrict__ covered, const u64 *__restrict__ cols, u64 wp, const i64 *__restrict__ res_idx,
                                                 i64 r0, i64 r1, unsigned first, unsigned n_local)
{
    for (u64 w = (u64)blockIdx.x * 256 + threadIdx.x; w < wp; w += (u64)gridDim.x * 256) {
        u64 acc = covered[w];
        for (i64 r = r0; r < r1; ++r) {  // (uniform)
            const i64 s = res_idx[r] - (i64)first;
            if (s >= 0 && s < (i64)n_local) acc |= cols[(u64)s * wp + w];
        }
        covered[w] = acc;
    }
}
