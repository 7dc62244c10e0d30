// Class counts: for a class label per variant, how many variants of every class each listed sample carries
// (utm_class_counts).
#pragma once
#include "common.hip.h"
#include "order.hip.h"
#include "swap.hip.h"

// ------------------------------------------------------------------------------------------------
// table[j][c] = |{v : column list[j] carries v and class[v] = c}|.  The classes partition the variants, so the work is
// bounded by the set bits of the listed columns (at most n x V), not by n_classes x n x V / 64 word operations as a
// bit-matrix product of n_classes class masks with the columns would be.
//
// Grid = (variant tile groups, column blocks of U listed columns), shaped like k_swap_pairs' grid with k_carrier_counts'
// decoding: a workgroup of four waves owns a 4 KiB tile of the variant axis at a time, a wave one KiB of it (one
// global_load_dwordx4 wave instruction per column), a lane 16 bytes = 128 variants.  The workgroup keeps U x n_classes
// 32-bit bins in LDS (at most UTM_CLASS_LDS_BINS = 16,384 of them, 64 KiB: U = min(16, 16384 / n_classes)), strides
// over the tiles of its group with the bins live and leaves with one 64-bit relaxed agent-scope atomic per non-zero bin.
// Integer sums: the order of the atomics cannot matter.  A workgroup walks at most UTM_SWAP_MAX_TILES_PER_WG tiles of
// 32,768 bits, so a 32-bit bin holds its sum.
//
// Per listed column the lane walks the set bits of its two words with ctz, reads the variant's label and adds 1 to bin
// (u, label) with an LDS atomic; a label of UTM_CLASS_NONE is skipped.  The NEXT column's 16 bytes are requested before
// this column's walk.  Labels: one uint16 per variant (n_classes <= 16,384; the host packs int32 -1 as UTM_CLASS_NONE),
// 64 per word of the column for every one of the wp words, so no load can leave the buffer; they are gathered from
// global memory, where a tile's 64 KiB of them are shared through L2 by every column block that walks the tile.
// ------------------------------------------------------------------------------------------------
#define UTM_CLASS_TILE_WORDS UTM_ORDER_TILE_WORDS  // a workgroup of four waves: 4 KiB of the variant axis
#define UTM_CLASS_U 16                             // listed columns per workgroup, at most
#define UTM_CLASS_LDS_BINS 16384                   // 32-bit bins a workgroup holds (64 KiB)
#define UTM_CLASS_NONE 0xFFFFu                     // the packed label of a variant that is counted nowhere

// An int32 label (-1 .. n_classes-1, n_classes <= UTM_CLASS_LDS_BINS) as the kernel reads it.
UTM_HD uint16_t class_pack(int32_t c) { return c < 0 ? (uint16_t)UTM_CLASS_NONE : (uint16_t)c; }
// Listed columns per workgroup for n_classes bins per column.
UTM_HD unsigned class_columns(unsigned n_classes)
{
    const unsigned u = UTM_CLASS_LDS_BINS / n_classes;
    return u < UTM_CLASS_U ? u : UTM_CLASS_U;
}
// The walk of one word: the lowest set bit of `todo`, which is cleared.
UTM_HD int class_next(u64 &todo)
{
    const int bit = __builtin_ctzll(todo);
    todo &= todo - 1;
    return bit;
}
// One word of one column into the column's n_classes bins: lab = the labels of the word's 64 variants.  Shared with the
// CPU build (BINS = plain sums there, LDS atomics here).
template <typename ADD>
UTM_HD void class_word(u64 w, const uint16_t *lab, ADD &&add)
{
    while (w) {
        const unsigned c = lab[class_next(w)];
        if (c != UTM_CLASS_NONE) add(c);
    }
}

// list: n column indices; cls: 64 * wp packed labels; table: n x n_classes sums, zeroed before the first launch.
// Dynamic LDS: U * n_classes * 4 bytes, U = class_columns(n_classes).  grid = (tile groups, ceil(n / U)); gridDim.x <=
// the number of tiles.
template <bool NT>
__global__ __launch_bounds__(256) void k_class_counts(const u64 *__restrict__ cols, u64 wp, const unsigned *__restrict__ list, unsigned n,
                                                      const uint16_t *__restrict__ cls, unsigned n_classes, u64 *__restrict__ table)
{
    extern __shared__ unsigned class_bins[];  // [u][class]
    const unsigned U = class_columns(n_classes);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const unsigned c0 = blockIdx.y * U;                     // the block's first listed column (< n by the grid)
    const unsigned nu = n - c0 < U ? n - c0 : U;            // ... and how many it has
    const unsigned n_bins = nu * n_classes;
    for (unsigned b = threadIdx.x; b < n_bins; b += 256) class_bins[b] = 0;
    __syncthreads();
    const u64 tiles = (wp + UTM_CLASS_TILE_WORDS - 1) / UTM_CLASS_TILE_WORDS;
    const u64 stride = wp / 2;  // a column, in 16-byte units
    for (u64 tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const u64 w0 = tile * UTM_CLASS_TILE_WORDS + (u64)wave * UTM_STEP_WORDS;
        // wp is a multiple of UTM_STEP_WORDS: a wave's KiB lies inside the column or past its end as a whole (no barrier
        // inside this loop)
        if (w0 >= wp) continue;
        const v2q *base = reinterpret_cast<const v2q *>(cols + w0) + lane;
        const uint16_t *lab = cls + (w0 + 2 * (u64)lane) * 64;  // the lane's 128 labels
#define UTM_CLASS_LOAD(I) (NT ? __builtin_nontemporal_load(base + (u64)list[c0 + (I)] * stride) : base[(u64)list[c0 + (I)] * stride])
        v2q x = UTM_CLASS_LOAD(0u);
        for (unsigned u = 0; u < nu; ++u) {
            v2q y = v2q{0, 0};
            if (u + 1 < nu) y = UTM_CLASS_LOAD(u + 1);  // (uniform)
            unsigned *bins = class_bins + u * n_classes;
            auto add = [bins](unsigned c) { atomicAdd(&bins[c], 1u); };
            class_word(x.x, lab, add);
            class_word(x.y, lab + 64, add);
            x = y;
        }
#undef UTM_CLASS_LOAD
    }
    __syncthreads();
    for (unsigned q = threadIdx.x; q < n_bins; q += 256)
        if (class_bins[q]) __hip_atomic_fetch_add(&table[(u64)c0 * n_classes + q], (u64)class_bins[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
