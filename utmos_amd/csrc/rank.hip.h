// Capture ranks: for a GIVEN list of samples, the position at which every variant is captured (utm_capture_rank).
#pragma once
#include "common.hip.h"
#include "depth.hip.h"
#include "order.hip.h"

// ------------------------------------------------------------------------------------------------
// rank[v] = the smallest i such that m of the columns o_0 .. o_i carry variant v, or -1 when the list never gets there
// (m = 1: the position of the first carrier).  One int32 per variant answers every prefix panel of the list at once:
// coverage after k samples = #(0 <= rank < k), the variants a panel of k misses = (rank < 0 or rank >= k).
//
// A sibling of k_order_curve without its sums: every 64-variant word is independent of every other, and nothing leaves
// a lane but the ranks of its own 128 variants -- no LDS, no barrier, no atomic.  A wave owns one KiB of the variant axis
// (one global_load_dwordx4 wave instruction per column), a lane 16 bytes of it; the lane keeps its two covered words and
// its 2 x P plane words (P = bit_length(m), depth.hip.h) in registers, starting from zero, and walks the list in rounds
// of UTM_RANK_U positions with the NEXT round's loads requested before this round's arithmetic (16 KiB in flight per
// wave: where k_order_curve landed, for the same reason -- a 10M-variant column is 1,224 waves on 1,024 SIMDs).
// Per position: depth_word<P> as it is, newly = covered after & ~covered before, and for every set bit of newly one
// 4-byte vector store of the position.  A variant saturates once, so it is written at most once; the buffer is filled
// with -1 before the launch.  Column padding is zero, so padding variants are never written.  Stores: at most 4 bytes
// per variant over the whole pass, next to n * wp * 8 bytes of loads.
// ------------------------------------------------------------------------------------------------
#define UTM_RANK_TILE_WORDS UTM_ORDER_TILE_WORDS  // a workgroup of four waves: 4 KiB of the variant axis
#define UTM_RANK_U UTM_ORDER_U

// One word of one column against the word's running state: the bits whose support reaches m with this column.  The
// whole arithmetic of a position, shared with the CPU build (utm_capture_rank_host).
template <int P>
UTM_HD u64 rank_word(u64 w, u64 &cov, u64 (&pl)[P], unsigned m)
{
    const u64 before = cov;
    unsigned units = 0, newly = 0;  // (depth_word's sums: not wanted here)
    depth_word<P>(w, cov, pl, m, units, newly);
    return cov & ~before;
}

// rank64[bit] = position for every set bit of `newly` (rank64 = the entry of the word's first variant).
UTM_HD void rank_store(int32_t *rank64, u64 newly, int32_t position)
{
    while (newly) {
        rank64[__builtin_ctzll(newly)] = position;
        newly &= newly - 1;
    }
}

// rank: 64 * wp entries (every word of the column has its 64, padding included), filled with -1.
template <int P, bool NT>
__global__ __launch_bounds__(256) void k_capture_rank(const u64 *__restrict__ cols, u64 wp, const unsigned *__restrict__ order, unsigned n,
                                                      unsigned m, int32_t *__restrict__ rank)
{
    constexpr int U = UTM_RANK_U;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const u64 w0 = (u64)blockIdx.x * UTM_RANK_TILE_WORDS + (u64)wave * UTM_STEP_WORDS;
    // wp is a multiple of UTM_STEP_WORDS: a wave's KiB lies inside the column or past its end as a whole (the waves of
    // the column's last tile; there is no barrier to keep them for)
    if (w0 >= wp) return;
    const v2q *base = reinterpret_cast<const v2q *>(cols + w0) + lane;
    const u64 stride = wp / 2;  // a column, in 16-byte units
    int32_t *mine = rank + (w0 + 2 * (u64)lane) * 64;  // the lane's 128 variants
#define UTM_RANK_LOAD(DST, I0)                                                                           \
    _Pragma("unroll") for (int u = 0; u < U; ++u) if ((I0) + u < n)                                      \
    {                                                                                                    \
        const v2q *p_ = base + (u64)order[(I0) + u] * stride;                                            \
        DST[u] = NT ? __builtin_nontemporal_load(p_) : *p_;                                              \
    }
    v2q x[U], y[U];
#pragma unroll
    for (int u = 0; u < U; ++u) x[u] = y[u] = v2q{0, 0};
    UTM_RANK_LOAD(x, 0u)
    u64 cov0 = 0, cov1 = 0, a[P], b[P];
#pragma unroll
    for (int p = 0; p < P; ++p) a[p] = b[p] = 0;
    for (unsigned i = 0; i < n; i += U) {
        if (i + U < n) { UTM_RANK_LOAD(y, i + U) }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (i + u < n) {  // (uniform)
                rank_store(mine, rank_word<P>(x[u].x, cov0, a, m), (int32_t)(i + u));
                rank_store(mine + 64, rank_word<P>(x[u].y, cov1, b, m), (int32_t)(i + u));
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) x[u] = y[u];
    }
#undef UTM_RANK_LOAD
}
