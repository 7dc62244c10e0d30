// Swap gains: what every exchange of one panel member for one other sample would capture (utm_swap_gains).
#pragma once
#include "common.hip.h"
#include "order.hip.h"

// ------------------------------------------------------------------------------------------------
// For a panel P = p_0 .. p_{k-1} with F(P) = the variants some member carries:
//
//     F(P - p_i + t) - F(P) = g_t + x[i][t] - u_i
//
// U_i = the variants ONLY member i carries (support exactly 1, in its column; the U_i are disjoint), u_i = |U_i|,
// g_t = popcount(col_t & ~covered), x[i][t] = popcount(col_t & U_i).  Taking p_i out loses U_i; bringing t in wins what
// nobody covered (g_t) and wins back what t carries of U_i.  No special case: t = p_i gives 0 + u_i - u_i, another member
// p_j gives 0 + 0 - u_i.
//
// Stage 1, k_swap_masks: one streaming pass over the k panel columns, shaped like k_capture_rank -- a lane owns 16 bytes
// of the variant axis and keeps a saturating two-plane counter per word in registers (swap_count).  It writes
// single = once & ~twice and uncov = ~once & valid (the padding bits of a column are zero in every column, but ~once has
// them set: they are cut here, once, so that no product below can count them).  k * wp * 8 bytes of loads.
//
// Stage 2, k_swap_pairs: a bit-matrix product, (k + 1) mask rows against n + 1 candidates over the chunk's words.  Mask
// row r < k is col_{p_r} & single, formed on the fly; row k is uncov, so its product with column t is g_t.  Candidate n
// is all ones: its product with row i is u_i, with row k it is the number of variants the panel misses.  Register
// blocked like a GEMM whose multiply-add is and + popcount:
//   - a lane owns ONE mask row (a wave = a block of 64 rows) and keeps UTM_SWAP_T int32 accumulators, one per candidate
//     of its block; nothing is ever reduced across lanes;
//   - a wave owns one KiB of a 4 KiB variant tile (as k_order_curve) and walks it in two halves: the half's candidate
//     words go into the wave's own 8 KiB of LDS with coalesced 16-byte loads (a wave instruction = 512 B of two
//     candidates), and come back with ds_read_b128 at a wave-uniform address -- a broadcast, no bank conflict;
//   - the lane's own row words come straight from global memory, 16 bytes per lane and load (64 columns, one line each;
//     the next seven loads hit the same lines), one load per 2 x UTM_SWAP_T candidate words;
//   - per 64 pair-bits: two v_and_b32 and two accumulating v_bcnt_u32_b32.
// The grid is (variant tile group, candidate block, row block); a workgroup strides over the tiles of its group with the
// accumulators live and adds them into x[(k + 1)][n + 1] (int64) with one vector atomic per (row, candidate) at its end.
// Integer sums: the order of the atomics cannot matter.
// ------------------------------------------------------------------------------------------------
#define UTM_SWAP_TILE_WORDS UTM_ORDER_TILE_WORDS  // a workgroup of four waves: 4 KiB of the variant axis
#define UTM_SWAP_T 16                             // candidates per block = accumulators per lane
#define UTM_SWAP_HALF (UTM_STEP_WORDS / 2)        // words of a wave's KiB staged at a time
#define UTM_SWAP_MAX_TILES_PER_WG 32768           // x 32,768 bits per tile and lane: an int32 accumulator holds it

// One word of one panel column against the word's two-plane counter (support saturating at 2).
UTM_HD void swap_count(u64 w, u64 &once, u64 &twice)
{
    twice |= once & w;
    once |= w;
}
// The variants exactly one panel member carries / the variants none carries (valid = the word's bits below n_var).
UTM_HD u64 swap_single(u64 once, u64 twice) { return once & ~twice; }
UTM_HD u64 swap_uncovered(u64 once, u64 valid) { return ~once & valid; }
// The bits of word w of a column that hold variants.
UTM_HD u64 swap_valid(u64 w, u64 n_var)
{
    return (w + 1) * 64 <= n_var ? ~0ull : w * 64 >= n_var ? 0ull : (1ull << (n_var & 63)) - 1;
}
// The multiply-add of the product: one mask word against one candidate word.
UTM_HD unsigned swap_pair(u64 row, u64 cand) { return (unsigned)__builtin_popcountll(row & cand); }

// single, uncov: wp words each (every word is written, padding words as 0).
__global__ __launch_bounds__(256) void k_swap_masks(const u64 *__restrict__ cols, u64 wp, u64 n_var, const unsigned *__restrict__ panel, unsigned k,
                                                    u64 *__restrict__ single, u64 *__restrict__ uncov)
{
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const u64 w0 = (u64)blockIdx.x * UTM_SWAP_TILE_WORDS + (u64)wave * UTM_STEP_WORDS;
    if (w0 >= wp) return;  // (wp is a multiple of UTM_STEP_WORDS: a wave's KiB lies inside the column or past it as a whole)
    const v2q *base = reinterpret_cast<const v2q *>(cols + w0) + lane;
    const u64 stride = wp / 2;  // a column, in 16-byte units
    u64 once0 = 0, once1 = 0, twice0 = 0, twice1 = 0;
#pragma unroll 8
    for (unsigned i = 0; i < k; ++i) {
        const v2q x = base[(u64)panel[i] * stride];
        swap_count(x.x, once0, twice0);
        swap_count(x.y, once1, twice1);
    }
    const u64 w = w0 + 2 * (u64)lane;
    reinterpret_cast<v2q *>(single + w0)[lane] = v2q{swap_single(once0, twice0), swap_single(once1, twice1)};
    reinterpret_cast<v2q *>(uncov + w0)[lane] = v2q{swap_uncovered(once0, swap_valid(w, n_var)), swap_uncovered(once1, swap_valid(w + 1, n_var))};
}

// x: (k + 1) x (n + 1) int64, row-major, zeroed before the first chunk's launch.  grid = (tile groups, candidate blocks,
// row blocks); gridDim.x <= the number of tiles.
__global__ __launch_bounds__(256) void k_swap_pairs(const u64 *__restrict__ cols, u64 wp, unsigned n, const unsigned *__restrict__ panel, unsigned k,
                                                    const u64 *__restrict__ single, const u64 *__restrict__ uncov, u64 *__restrict__ x)
{
    constexpr int T = UTM_SWAP_T, H = UTM_SWAP_HALF;
    __shared__ v2q cand[4][T][H / 2];  // [wave][candidate][16-byte unit of the half]: 8 KiB per wave
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const unsigned r = blockIdx.z * 64 + lane;   // the lane's mask row
    const unsigned t0 = blockIdx.y * T;          // the block's first candidate
    const u64 tiles = (wp + UTM_SWAP_TILE_WORDS - 1) / UTM_SWAP_TILE_WORDS;
    // row r < k: the member's column under `single`; row k: uncov as it is; rows past k (the last block's idle lanes)
    // read uncov too and are masked to 0
    const u64 *rowp = r < k ? cols + (u64)panel[r] * wp : uncov;
    const bool member = r < k, live = r <= k;
    // staging: lane -> (candidate of a pair, 16-byte unit); a wave instruction brings 512 B of each of two candidates
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
                    else if (t == n) v = v2q{~0ull, ~0ull};  // the all-ones candidate: row sums
                    cand[wave][2 * q + st_c][st_u] = v;
                }
            }
            __syncthreads();
            if (own) {
                const v2q *rp = reinterpret_cast<const v2q *>(rowp + wh);
                const v2q *sp = reinterpret_cast<const v2q *>(single + wh);
#pragma unroll 4
                for (int u = 0; u < H / 2; ++u) {
                    v2q row = rp[u];
                    const v2q s = sp[u];  // (wave-uniform address)
                    row.x = member ? row.x & s.x : live ? row.x : 0ull;
                    row.y = member ? row.y & s.y : live ? row.y : 0ull;
#pragma unroll
                    for (int t = 0; t < T; ++t) {
                        const v2q c = cand[wave][t][u];
                        acc[t] += (int)(swap_pair(row.x, c.x) + swap_pair(row.y, c.y));
                    }
                }
            }
        }
    }
    if (!live) return;
    u64 *xr = x + (u64)r * (n + 1);
#pragma unroll
    for (int t = 0; t < T; ++t)
        if (t0 + t <= n && acc[t]) atomicAdd(&xr[t0 + t], (u64)acc[t]);
}
