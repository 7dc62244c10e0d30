// Replicated selection: B greedy selections at once, each over its own subset of the variants and with its own sample
// states (utm_multi_select).
#pragma once
#include "common.hip.h"
#include "order.hip.h"
#include "swap.hip.h"

// ------------------------------------------------------------------------------------------------
// Replicate b keeps a live mask live_b (one bit per variant of the chunk: kept by the replicate and not captured yet) and
// a state byte per sample.  One iteration of all replicates:
//
//   k_multi_score   scores[t][b] += popcount(col_t & live_b) over the chunk's words -- the bit-matrix product of
//                   k_swap_pairs with the mask rows read from the live buffer: a lane owns ONE replicate (a wave = a block
//                   of 64 replicates) and UTM_SWAP_T int32 accumulators, the candidate words of a half KiB are staged per
//                   wave in LDS and come back as broadcasts, a workgroup strides over the tiles of its group.  At its end
//                   the four waves' accumulators meet in LDS and every (candidate, replicate) cell gets ONE 64-bit vector
//                   atomic; the scores are stored [candidate][replicate], so that a wave's atomic covers 512 contiguous
//                   bytes.  With B < 64 replicates only B lanes of a row block do work: the launch costs what 64 cost.
//   k_multi_pick    per replicate the first maximum over its selectable samples; writes the row, marks the winner used,
//                   ends the replicate (best score 0, or its last kept variant captured) and clears the score cells.
//   k_multi_apply   live_b &= ~col_winner_b.
//
// k_multi_keep writes the hashed masks, k_multi_init turns the masks into live masks and counts the kept variants.
// Every kernel returns at once when no replicate is left (MultiCtl::left == 0).
// ------------------------------------------------------------------------------------------------
#define UTM_MULTI_MAX_REP 256

struct MultiCtl {
    int left;  // replicates still running
    int pad;
};

// Does variant v (counted from 0 over all chunks) belong to replicate b?  splitmix64 of seed, v and b; the top 32 bits
// against the threshold (2^32 keeps everything).
UTM_HD u64 multi_hash(u64 seed, u64 v, u64 b)
{
    return utm_mix64(seed + 0x9E3779B97F4A7C15ull * (v + 1) + 0xD1B54A32D192ED03ull * (b + 1));
}
UTM_HD bool multi_keeps(u64 seed, u64 v, u64 b, u64 threshold) { return (multi_hash(seed, v, b) >> 32) < threshold; }
// The keep word of 64 consecutive variants from v0 on, of which `bits` (0..64) exist.
UTM_HD u64 multi_keep_word(u64 seed, u64 b, u64 v0, unsigned bits, u64 threshold)
{
    u64 word = 0;
    for (unsigned i = 0; i < bits; ++i) word |= (u64)multi_keeps(seed, v0 + i, b, threshold) << i;
    return word;
}
// A replicate's live word at its start: kept, a variant, and carried by none of its used samples.
UTM_HD u64 multi_live(u64 keep, u64 valid, u64 used_or) { return keep & valid & ~used_or; }
// First maximum: does (score, idx) beat (best, best_idx)?  best_idx < 0: nothing yet.
UTM_HD bool multi_better(i64 score, i64 idx, i64 best, i64 best_idx)
{
    return best_idx < 0 || score > best || (score == best && idx < best_idx);
}

// live[b * wp + w] of one chunk (every word of the first `words` is written; the padding stays as the caller cleared it).
// grid = (ceil(words / 256), n_rep)
__global__ __launch_bounds__(256) void k_multi_keep(u64 *__restrict__ live, u64 wp, u64 words, u64 n_var, u64 first_var_global, u64 seed, u64 threshold)
{
    const u64 w = (u64)blockIdx.x * 256 + threadIdx.x;
    if (w >= words) return;
    const unsigned b = blockIdx.y;
    const u64 left = n_var - w * 64;
    live[(u64)b * wp + w] = multi_keep_word(seed, b, first_var_global + w * 64, left < 64 ? (unsigned)left : 64u, threshold);
}

// live[b][w] (holding the replicate's keep words) -> its live words; kept[b] += the replicate's variants in this chunk.
// used_idx[used_off[b] .. used_off[b + 1]): the replicate's used samples.  grid = (wp / 512, n_rep): a lane owns 16 bytes.
__global__ __launch_bounds__(256) void k_multi_init(const u64 *__restrict__ cols, u64 wp, u64 n_var, u64 *__restrict__ live,
                                                   const unsigned *__restrict__ used_off, const unsigned *__restrict__ used_idx, u64 *__restrict__ kept)
{
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const unsigned b = blockIdx.y;
    const u64 w0 = (u64)blockIdx.x * UTM_SWAP_TILE_WORDS + (u64)wave * UTM_STEP_WORDS;
    if (w0 >= wp) return;  // (wp is a multiple of UTM_STEP_WORDS)
    v2q *lp = reinterpret_cast<v2q *>(live + (u64)b * wp + w0) + lane;
    const v2q *base = reinterpret_cast<const v2q *>(cols + w0) + lane;
    const u64 stride = wp / 2;
    v2q keep = *lp;
    const u64 w = w0 + 2 * (u64)lane;
    keep.x &= swap_valid(w, n_var);
    keep.y &= swap_valid(w + 1, n_var);
    const unsigned n_kept = wave_sum_u32((unsigned)(__builtin_popcountll(keep.x) + __builtin_popcountll(keep.y)));
    if (lane == 0 && n_kept) atomicAdd(&kept[b], (u64)n_kept);
    u64 or0 = 0, or1 = 0;
    const unsigned lo = used_off[b], hi = used_off[b + 1];
#pragma unroll 4
    for (unsigned i = lo; i < hi; ++i) {
        const v2q x = base[(u64)used_idx[i] * stride];
        or0 |= x.x;
        or1 |= x.y;
    }
    *lp = v2q{multi_live(keep.x, ~0ull, or0), multi_live(keep.y, ~0ull, or1)};
}

// scores: [n][rb] int64 (rb = row blocks x 64), all zero before the first chunk's launch of an iteration.
// grid = (tile groups, candidate blocks, row blocks); gridDim.x <= the number of tiles.
__global__ __launch_bounds__(256) void k_multi_score(const u64 *__restrict__ cols, u64 wp, unsigned n, const u64 *__restrict__ live, unsigned n_rep,
                                                    const unsigned char *__restrict__ done, const MultiCtl *__restrict__ ctl, u64 *__restrict__ scores,
                                                    unsigned rb)
{
    constexpr int T = UTM_SWAP_T, H = UTM_SWAP_HALF;
    __shared__ v2q cand[4][T][H / 2];  // [wave][candidate][16-byte unit of the half]: 8 KiB per wave
    if (ctl->left == 0) return;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const unsigned r = blockIdx.z * 64 + lane;   // the lane's replicate
    const unsigned t0 = blockIdx.y * T;          // the block's first candidate
    const bool alive = r < n_rep && !done[r < n_rep ? r : 0];
    // every wave of the block holds the same 64 replicates: the vote is the same in all four, so all leave or none does
    if (!__builtin_amdgcn_readfirstlane((int)(__ballot(alive) != 0))) return;
    const u64 tiles = (wp + UTM_SWAP_TILE_WORDS - 1) / UTM_SWAP_TILE_WORDS;
    const u64 *rowp = live + (u64)(alive ? r : 0) * wp;  // (idle lanes read row 0 and are masked to 0)
    const int st_c = lane >> 5, st_u = lane & 31;
    int acc[T];
#pragma unroll
    for (int t = 0; t < T; ++t) acc[t] = 0;
    for (u64 tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const u64 w0 = tile * UTM_SWAP_TILE_WORDS + (u64)wave * UTM_STEP_WORDS;
        const bool own = w0 < wp;  // a wave past the column's end (its last tile) stages and counts nothing, but keeps the barriers
        for (int half = 0; half < 2; ++half) {
            const u64 wh = w0 + (u64)half * H;
            __syncthreads();  // the previous half's readers are done with the wave's LDS
            if (own) {
#pragma unroll
                for (int q = 0; q < T / 2; ++q) {
                    const unsigned t = t0 + 2 * q + st_c;
                    v2q v = v2q{0, 0};
                    if (t < n) v = reinterpret_cast<const v2q *>(cols + (u64)t * wp + wh)[st_u];
                    cand[wave][2 * q + st_c][st_u] = v;
                }
            }
            __syncthreads();
            if (own) {
                const v2q *rp = reinterpret_cast<const v2q *>(rowp + wh);
#pragma unroll 4
                for (int u = 0; u < H / 2; ++u) {
                    v2q row = rp[u];
                    row.x = alive ? row.x : 0ull;
                    row.y = alive ? row.y : 0ull;
#pragma unroll
                    for (int t = 0; t < T; ++t) {
                        const v2q c = cand[wave][t][u];
                        acc[t] += (int)(swap_pair(row.x, c.x) + swap_pair(row.y, c.y));
                    }
                }
            }
        }
    }
    // the four waves counted the same (replicate, candidate) cells over different KiB: sum them in LDS, one atomic per cell
    __syncthreads();
    int *red = reinterpret_cast<int *>(&cand[0][0][0]);  // [wave][T][64] ints: 16 of the 32 KiB
#pragma unroll
    for (int t = 0; t < T; ++t) red[(wave * T + t) * 64 + lane] = acc[t];
    __syncthreads();
#pragma unroll
    for (int j = 0; j < T / 4; ++j) {
        const int t = wave * (T / 4) + j;
        const int sum = red[(0 * T + t) * 64 + lane] + red[(1 * T + t) * 64 + lane] + red[(2 * T + t) * 64 + lane] + red[(3 * T + t) * 64 + lane];
        if (alive && t0 + t < n && sum) atomicAdd(&scores[(u64)(t0 + t) * rb + r], (u64)sum);
    }
}

struct MultiPick {
    u64 *scores;            // [n][rb]
    unsigned char *state;   // [n_rep][n]: the call's own copy, winners become 0
    unsigned char *done;    // [n_rep]
    int *winner;            // [n_rep]: the column k_multi_apply takes out, or -1
    int *order;             // [n_rep][k]
    i64 *gain;              // [n_rep][k]
    i64 *rows;              // [n_rep]: rows written
    i64 *tot;               // [n_rep]: variants captured by them
    const u64 *kept;        // [n_rep]
    MultiCtl *ctl;
    unsigned n, rb;
    i64 k;
};

// grid = n_rep blocks of 256 threads
__global__ __launch_bounds__(256) void k_multi_pick(MultiPick a)
{
    __shared__ i64 s_score[4];
    __shared__ i64 s_idx[4];
    if (a.ctl->left == 0) return;
    const unsigned b = blockIdx.x;
    if (a.done[b]) return;  // (its score cells were never added to: still 0)
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const unsigned char *st = a.state + (u64)b * a.n;
    i64 best = 0, best_idx = -1;
    for (unsigned s = threadIdx.x; s < a.n; s += 256) {
        u64 *cell = a.scores + (u64)s * a.rb + b;
        const i64 v = (i64)*cell;
        *cell = 0;  // for the next iteration's atomics
        if (st[s] == 1 && multi_better(v, s, best, best_idx)) {
            best = v;
            best_idx = s;
        }
    }
    for (int d = 1; d < 64; d <<= 1) {
        const i64 o = __shfl_xor(best, d), oi = __shfl_xor(best_idx, d);
        if (oi >= 0 && multi_better(o, oi, best, best_idx)) {
            best = o;
            best_idx = oi;
        }
    }
    if (lane == 0) {
        s_score[wave] = best;
        s_idx[wave] = best_idx;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int w = 1; w < 4; ++w)
        if (s_idx[w] >= 0 && multi_better(s_score[w], s_idx[w], best, best_idx)) {
            best = s_score[w];
            best_idx = s_idx[w];
        }
    bool ends = false;
    a.winner[b] = -1;
    if (best_idx < 0 || best == 0) {
        ends = true;  // silently: no row
    } else {
        const i64 row = a.rows[b];
        a.order[(u64)b * a.k + row] = (int)best_idx;
        a.gain[(u64)b * a.k + row] = best;
        a.rows[b] = row + 1;
        a.tot[b] += best;
        a.state[(u64)b * a.n + best_idx] = 0;
        if (a.tot[b] >= (i64)a.kept[b] || row + 1 >= a.k) ends = true;  // the row that captures the last kept variant, or the k-th
        else a.winner[b] = (int)best_idx;
    }
    if (ends) {
        a.done[b] = 1;
        atomicSub(&a.ctl->left, 1);
    }
}

// grid = (wp / 512, n_rep)
__global__ __launch_bounds__(256) void k_multi_apply(const u64 *__restrict__ cols, u64 wp, u64 *__restrict__ live, const int *__restrict__ winner,
                                                    const MultiCtl *__restrict__ ctl)
{
    if (ctl->left == 0) return;
    const unsigned b = blockIdx.y;
    const int win = winner[b];
    if (win < 0) return;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const u64 w0 = (u64)blockIdx.x * UTM_SWAP_TILE_WORDS + (u64)wave * UTM_STEP_WORDS;
    if (w0 >= wp) return;
    v2q *lp = reinterpret_cast<v2q *>(live + (u64)b * wp + w0) + lane;
    const v2q c = (reinterpret_cast<const v2q *>(cols + (u64)win * wp + w0))[lane];
    v2q l = *lp;
    l.x &= ~c.x;
    l.y &= ~c.y;
    *lp = l;
}
