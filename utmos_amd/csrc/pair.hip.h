// Pair counts: the variants every two samples of a list share (utm_pair_counts).
#pragma once
#include "common.hip.h"
#include "order.hip.h"
#include "swap.hip.h"

// ------------------------------------------------------------------------------------------------
// For a list idx[0..n) of columns and an optional mask word stream (uncov of k_swap_masks(panel = given): the variants
// no `given` sample carries, valid-bit cut included):
//
//     x[i][j] = sum over the words of popcount(col[idx[i]] & col[idx[j]] & mask)
//
// a symmetric bit-matrix product whose BOTH operands are blocks of columns.  k_swap_pairs gives a lane one mask row read
// from global memory; here both operands of a 64 x 64 block pair are staged in LDS and every lane keeps a 4 x 4
// sub-block of it in registers, so one LDS read feeds four multiply-adds (and + popcount, swap_pair):
//   - a workgroup of four waves owns one block pair (bi, bj >= bi) and a group of 4 KiB variant tiles
//     (UTM_ORDER_TILE_WORDS); it walks a tile in slices of UTM_PAIR_SLICE words;
//   - staging: thread t brings 16 bytes: unit u = t & 7 of the slice (UTM_PAIR_UNITS = 8 units of two words) of sample
//     t >> 3 and of sample 32 + (t >> 3), for the row block and -- unless bi == bj, which stages once and reads it
//     twice -- the column block: eight consecutive lanes read 128 contiguous bytes of one column.  The mask is and-ed
//     into the column operand on the way (ONE operand: a diagonal block stages only that one); without a mask there
//     is no mask load.  List positions >= n stage zeros.  The NEXT slice's loads are issued before this
//     slice's arithmetic, so their latency runs under 1,024 VALU instructions per wave;
//   - LDS image of an operand: 16-byte slot (u * 64 + (s ^ u)) holds unit u of block sample s, 8 KiB per operand;
//   - the 256 lanes are a 16 x 16 grid (ti = t >> 4, tj = t & 15); a lane owns rows ti + 16 a and columns tj + 16 b
//     (a, b = 0..3).  Per unit it reads 4 row slots and 4 column slots with ds_read_b128 (8 reads, 128 bytes) for 32
//     word pairs = 128 VALU instructions (two v_and_b32 and two accumulating v_bcnt_u32_b32 per word pair).
// Why the reads are conflict-free: ds_read_b128 is served in four groups of 16 lanes, banks = the 16 slots of a 256-byte
// row.  A column read (fixed u, b) addresses slot 64 u + 16 b + (tj ^ u): every one of the four lane groups holds each
// tj = 0..15 once, and x -> x ^ u (u < 8) permutes 0..15, so a group reads 16 different slots of ONE 256-byte row.  A
// row read (fixed u, a) has one address per ti; a wave holds four consecutive ti, a lane group two of them (two slots of
// one row, different banks) -- everything else is a broadcast.  The staging store ds_write_b128 is served in groups of 8
// consecutive lanes over 32 banks = 8 slots: those lanes hold one sample and u = 0..7, i.e. slots (s ^ u) & 7 -- all
// eight.  The xor exists for the store; the reads do not need it and do not suffer from it.
// A workgroup strides over the tiles of its group with the 16 accumulators live (at most UTM_SWAP_MAX_TILES_PER_WG
// tiles: 2^15 tiles x 2^15 bits stay inside an int32) and ends with one 64-bit vector atomic per (i, j) with a nonzero
// sum.  Integer sums: the order of the atomics cannot matter.  Only bj >= bi is launched; a diagonal block computes all
// of its 64 x 64, the host mirrors the blocks above the diagonal.
// grid = (block pairs, tile groups): the block pairs are the fast index, so the workgroups in flight together walk the
// SAME tiles and a column block's slice comes out of HBM once and out of the caches for the other block pairs.
// ------------------------------------------------------------------------------------------------
#define UTM_PAIR_B 64         // samples of a block
#define UTM_PAIR_SLICE 16     // words of a column staged at a time
#define UTM_PAIR_UNITS (UTM_PAIR_SLICE / 2)
static_assert(UTM_STEP_WORDS % UTM_PAIR_SLICE == 0 && UTM_PAIR_UNITS == 8, "a column (a multiple of UTM_STEP_WORDS) is whole slices; 8 units = 8 lanes of a store group");

// One word of an operand under the mask, as it is staged.
UTM_HD u64 pair_stage(u64 w, u64 mask) { return w & mask; }
// The 16-byte slot of unit u of block sample s inside an operand's LDS image.
UTM_HD unsigned pair_slot(unsigned u, unsigned s) { return u * UTM_PAIR_B + (s ^ u); }
// Block pair p of the nb (nb + 1) / 2 pairs bj >= bi, row by row.
UTM_HD void pair_blocks(unsigned p, unsigned nb, unsigned &bi, unsigned &bj)
{
    bi = 0;
    while (p >= nb - bi) {
        p -= nb - bi;
        ++bi;
    }
    bj = bi + p;
}

// x: n x n int64, row-major, zeroed before the first chunk's launch; only the blocks bj >= bi are written.
// grid = (nb (nb + 1) / 2, tile groups), gridDim.y <= the number of tiles.  uncov: wp words, or nullptr.
template <bool NT>
__global__ __launch_bounds__(256) void k_pair_counts(const u64 *__restrict__ cols, u64 wp, const unsigned *__restrict__ idx, unsigned n,
                                                     const u64 *__restrict__ uncov, u64 *__restrict__ x)
{
    constexpr int B = UTM_PAIR_B, U = UTM_PAIR_UNITS;
    __shared__ v2q img[2][U * B];  // [row operand, column operand][slot]: 8 KiB each
    const unsigned t = threadIdx.x;
    unsigned bi, bj;
    pair_blocks(blockIdx.x, (n + B - 1) / B, bi, bj);
    const bool diag = bi == bj, masked = uncov != nullptr;
    const u64 tiles = (wp + UTM_ORDER_TILE_WORDS - 1) / UTM_ORDER_TILE_WORDS;

    // staging: this thread's unit and its two samples of either block
    const unsigned st_u = t & (U - 1), st_s = t >> 3;
    const v2q *src[4];  // [row block: samples st_s, st_s + 32][column block: the same], nullptr past the list
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const unsigned pos = (q < 2 ? bi : bj) * B + st_s + 32 * (q & 1);
        src[q] = pos < n ? reinterpret_cast<const v2q *>(cols + (u64)idx[pos] * wp) + st_u : nullptr;
    }
    const v2q *msk = masked ? reinterpret_cast<const v2q *>(uncov) + st_u : nullptr;
    v2q held[4];
    // the slice at word w of every column -> registers (the mask goes into the column operand, the one every block stages)
#define UTM_PAIR_LOAD(W)                                                                                             \
    {                                                                                                                \
        const u64 unit_ = (W) / 2;                                                                                   \
        v2q m_ = v2q{~0ull, ~0ull};                                                                                  \
        if (masked) m_ = msk[unit_];                                                                                 \
        _Pragma("unroll") for (int q = 0; q < 4; ++q)                                                                \
        {                                                                                                            \
            v2q v_ = v2q{0, 0};                                                                                      \
            if (src[q] && (q >= 2 || !diag)) v_ = NT ? __builtin_nontemporal_load(src[q] + unit_) : src[q][unit_];   \
            if (q >= 2) v_ = v2q{pair_stage(v_.x, m_.x), pair_stage(v_.y, m_.y)};                                    \
            held[q] = v_;                                                                                            \
        }                                                                                                            \
    }

    // arithmetic: this lane's 4 x 4 sub-block
    const unsigned ti = t >> 4, tj = t & 15;
    const v2q *rows = img[diag ? 1 : 0], *cands = img[1];
    int acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = 0;

    u64 tile = blockIdx.y;
    u64 w = tile * UTM_ORDER_TILE_WORDS, end = w + UTM_ORDER_TILE_WORDS < wp ? w + UTM_ORDER_TILE_WORDS : wp;  // (tile < tiles: w < wp)
    if (tile < tiles) UTM_PAIR_LOAD(w)
    while (tile < tiles) {
        __syncthreads();  // the previous slice's readers are done with the images
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (q >= 2 || !diag) img[q >> 1][pair_slot(st_u, st_s + 32 * (q & 1))] = held[q];
        __syncthreads();
        // on to the next slice (of this tile, or the first of the group's next tile): its loads fly during the arithmetic
        w += UTM_PAIR_SLICE;
        if (w >= end) {
            tile += gridDim.y;
            w = tile * UTM_ORDER_TILE_WORDS;
            end = w + UTM_ORDER_TILE_WORDS < wp ? w + UTM_ORDER_TILE_WORDS : wp;
        }
        if (tile < tiles) UTM_PAIR_LOAD(w)
#pragma unroll
        for (int u = 0; u < U; ++u) {
            v2q r[4], c[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) r[a] = rows[pair_slot(u, ti + 16 * a)];
#pragma unroll
            for (int b = 0; b < 4; ++b) c[b] = cands[pair_slot(u, tj + 16 * b)];
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) acc[a][b] += (int)(swap_pair(r[a].x, c[b].x) + swap_pair(r[a].y, c[b].y));
        }
    }
#undef UTM_PAIR_LOAD
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const unsigned i = bi * B + ti + 16 * a;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const unsigned j = bj * B + tj + 16 * b;
            if (i < n && j < n && acc[a][b]) atomicAdd(&x[(u64)i * n + j], (u64)acc[a][b]);
        }
    }
}
