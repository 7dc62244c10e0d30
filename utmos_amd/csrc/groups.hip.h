// Group curves: for a GIVEN list of samples and a population label per sample, what every prefix of the list captures of
// the variants each population carries (utm_group_curve).
#pragma once
#include "common.hip.h"
#include "order.hip.h"

// ------------------------------------------------------------------------------------------------
// U_g = the variants some sample of group g carries, multi = the variants in two or more U_g, P_g = U_g & ~multi (the
// group's private variants).  new[g][j] = the variants of U_g whose first carrier in the list stands at position j (the
// rank of k_capture_rank at m = 1), priv[g][j] the same over P_g, total[g] = |U_g|, ptotal[g] = |P_g|.
//
// Two streaming passes, both in the launch shape of k_capture_rank and k_carrier_counts: a workgroup of four waves owns a
// 4 KiB tile of the variant axis, a wave one KiB of it (one global_load_dwordx4 wave instruction per column), a lane 16
// bytes; the columns come in rounds of UTM_GROUP_U = 16 with the NEXT round's loads requested before this round's
// arithmetic.
//
// k_group_unions: one pass over the columns of all grouped samples, which the host hands over sorted by group with G + 1
// offsets.  The lane ORs a group's columns into a running word pair; where the list passes an offset (wave-uniform) the
// pair is stored as the group's union word and folded into a saturating two-plane counter over the GROUPS (group_close:
// once, twice), so `twice` ends as multi.  Masks: (G + 1) rows of wp words, row G = multi; every word of every row is
// written.  No LDS, no atomics on that path.  The totals are popcounts of the lane's own mask words (read back once the
// multi word is known), summed per wave by the DPP ladder: one 64-bit atomic per wave, group and sum, skipped at 0.
//
// k_group_curve: the walk of k_capture_rank<1> over the order: newly = column & ~covered per position, in registers.
// Only where a lane's newly is non-zero does it read its 16 bytes of the G union rows (and of multi, PRIV) and add
// popcount(newly & U_g) to bin (g, position): a variant is captured once, so a lane gets there at most 128 times whatever
// n and G are -- the work beyond the column loads is bounded by the captures.  Under a greedy or a random order almost
// everything is captured by the first positions, so the positions below R meet in LDS bins (32 bits: a tile has 32,768
// variants; R = UTM_GROUP_LDS_BINS / bin rows, at most n) and leave with one 64-bit global atomic per non-zero bin; the
// positions from R on add to the global bins directly (few captures, spread addresses).  A group's never-captured count
// is total - sum_j new: it is no bin, so it can never be a hot address.  Integer sums: the order of the atomics cannot
// matter.
// ------------------------------------------------------------------------------------------------
#define UTM_GROUP_TILE_WORDS UTM_ORDER_TILE_WORDS  // a workgroup of four waves: 4 KiB of the variant axis
#define UTM_GROUP_U UTM_ORDER_U
#define UTM_GROUP_LDS_BINS 8192                    // 32 KiB of head bins: 3 workgroups of a CU hold theirs at once

// One word of one column against the word's covered state: the bits this column captures (rank_word at m = 1 without
// its planes).
UTM_HD u64 group_newly(u64 w, u64 &cov)
{
    const u64 newly = w & ~cov;
    cov |= w;
    return newly;
}
// A finished union word into the two-plane counter over the groups.
UTM_HD void group_close(u64 u, u64 &once, u64 &twice)
{
    twice |= once & u;
    once |= u;
}
UTM_HD u64 group_private(u64 u, u64 multi) { return u & ~multi; }
// What a position's captures add to a group's bin.
UTM_HD unsigned group_hits(u64 newly, u64 u) { return (unsigned)__builtin_popcountll(newly & u); }

// The number of head positions the LDS bins hold for `rows` bin rows and a list of n.
UTM_HD unsigned group_head(unsigned rows, u64 n)
{
    const u64 r = UTM_GROUP_LDS_BINS / rows;
    return (unsigned)(n < r ? n : r);
}

// list: the grouped samples sorted by group, offs[g] .. offs[g + 1] = group g's; masks: (G + 1) x wp words, all written;
// totals: 2 x G sums (|U_g|, then |P_g|), zeroed before the launch.
template <bool NT>
__global__ __launch_bounds__(256) void k_group_unions(const u64 *__restrict__ cols, u64 wp, const unsigned *__restrict__ list,
                                                      const unsigned *__restrict__ offs, unsigned G, u64 *masks, u64 *__restrict__ totals)
{
    constexpr int U = UTM_GROUP_U;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const u64 w0 = (u64)blockIdx.x * UTM_GROUP_TILE_WORDS + (u64)wave * UTM_STEP_WORDS;
    // wp is a multiple of UTM_STEP_WORDS: a wave's KiB lies inside the column or past its end as a whole (no barrier here)
    if (w0 >= wp) return;
    const v2q *base = reinterpret_cast<const v2q *>(cols + w0) + lane;
    const u64 stride = wp / 2;  // a column or a mask row, in 16-byte units
    v2q *mine = reinterpret_cast<v2q *>(masks + w0) + lane;  // the lane's unit of row 0
    const unsigned n = offs[G];
#define UTM_GROUP_LOAD(DST, I0)                                                                          \
    _Pragma("unroll") for (int u = 0; u < U; ++u) if ((I0) + u < n)                                      \
    {                                                                                                    \
        const v2q *p_ = base + (u64)list[(I0) + u] * stride;                                             \
        DST[u] = NT ? __builtin_nontemporal_load(p_) : *p_;                                              \
    }
    v2q x[U], y[U];
#pragma unroll
    for (int u = 0; u < U; ++u) x[u] = y[u] = v2q{0, 0};
    UTM_GROUP_LOAD(x, 0u)
    u64 u0 = 0, u1 = 0, once0 = 0, once1 = 0, twice0 = 0, twice1 = 0;
    unsigned g = 0, end = offs[1];
#define UTM_GROUP_CLOSE()                                                                                \
    {                                                                                                    \
        mine[(u64)g * stride] = v2q{u0, u1};                                                             \
        group_close(u0, once0, twice0);                                                                  \
        group_close(u1, once1, twice1);                                                                  \
        u0 = u1 = 0;                                                                                     \
        ++g;                                                                                             \
    }
    for (unsigned i = 0; i < n; i += U) {
        if (i + U < n) { UTM_GROUP_LOAD(y, i + U) }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (i + u < n) {  // (uniform)
                // position i + u < offs[G] opens a later group: g + 1 < G after the close, so offs[g + 1] exists
                while (i + u == end) {
                    UTM_GROUP_CLOSE()
                    end = offs[g + 1];
                }
                u0 |= x[u].x;
                u1 |= x[u].y;
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) x[u] = y[u];
    }
    while (g < G) UTM_GROUP_CLOSE()  // the last group with samples, and every empty one behind it
#undef UTM_GROUP_CLOSE
#undef UTM_GROUP_LOAD
    mine[(u64)G * stride] = v2q{twice0, twice1};
    for (unsigned q = 0; q < G; ++q) {  // (all 64 lanes are here: the DPP sums are whole)
        const v2q m = mine[(u64)q * stride];  // the lane's own store
        const unsigned t = wave_sum_u32((unsigned)(__builtin_popcountll(m.x) + __builtin_popcountll(m.y)));
        const unsigned p = wave_sum_u32((unsigned)(__builtin_popcountll(group_private(m.x, twice0)) + __builtin_popcountll(group_private(m.y, twice1))));
        if (lane == 0 && t) __hip_atomic_fetch_add(&totals[q], (u64)t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (lane == 0 && p) __hip_atomic_fetch_add(&totals[G + q], (u64)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// One bin: positions below R in the workgroup's LDS head, the others in the global bins.
__device__ __forceinline__ void group_bin(unsigned row, unsigned pos, unsigned add, unsigned n, unsigned R, unsigned *head, u64 *bins)
{
    if (pos < R) atomicAdd(&head[row * R + pos], add);
    else atomicAdd(&bins[(u64)row * n + pos], (u64)add);
}

// A position's captures of one lane (newly0 | newly1 != 0) into the bins of every group that has some of them.
// mk: the lane's 16 bytes of mask row 0.
template <bool PRIV>
__device__ __forceinline__ void group_add(u64 newly0, u64 newly1, const v2q *mk, u64 stride, unsigned G, unsigned pos, unsigned n, unsigned R,
                                          unsigned *head, u64 *bins)
{
    u64 p0 = newly0, p1 = newly1;
    if (PRIV) {
        const v2q multi = mk[(u64)G * stride];
        p0 = group_private(newly0, multi.x);
        p1 = group_private(newly1, multi.y);
    }
    for (unsigned g = 0; g < G; ++g) {
        const v2q u = mk[(u64)g * stride];
        const unsigned c = group_hits(newly0, u.x) + group_hits(newly1, u.y);
        if (c) group_bin(g, pos, c, n, R, head, bins);
        if (PRIV) {
            const unsigned p = group_hits(p0, u.x) + group_hits(p1, u.y);
            if (p) group_bin(G + g, pos, p, n, R, head, bins);
        }
    }
}

// masks: (G + 1) x wp words of k_group_unions (row G is read under PRIV only); bins: (PRIV ? 2 G : G) x n sums, row G + g
// = group g's private bins, zeroed before the launch.  R <= n head positions meet in LDS ((PRIV ? 2 G : G) * R <=
// UTM_GROUP_LDS_BINS), 0 = none.
template <bool PRIV, bool NT>
__global__ __launch_bounds__(256) void k_group_curve(const u64 *__restrict__ cols, u64 wp, const unsigned *__restrict__ order, unsigned n,
                                                     const u64 *__restrict__ masks, unsigned G, unsigned R, u64 *__restrict__ bins)
{
    constexpr int U = UTM_GROUP_U;
    __shared__ unsigned head[UTM_GROUP_LDS_BINS];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const u64 w0 = (u64)blockIdx.x * UTM_GROUP_TILE_WORDS + (u64)wave * UTM_STEP_WORDS;
    // wp is a multiple of UTM_STEP_WORDS: a wave's KiB lies inside the column or past its end as a whole.  A wave past
    // it (the column's last tile) loads and counts nothing, but keeps the barriers.
    const bool own = w0 < wp;
    const unsigned n_head = (PRIV ? 2 * G : G) * R;
    for (unsigned b = threadIdx.x; b < n_head; b += 256) head[b] = 0;
    __syncthreads();
    if (own) {
        const v2q *base = reinterpret_cast<const v2q *>(cols + w0) + lane;
        const v2q *mk = reinterpret_cast<const v2q *>(masks + w0) + lane;
        const u64 stride = wp / 2;  // a column or a mask row, in 16-byte units
#define UTM_GROUP_LOAD(DST, I0)                                                                          \
    _Pragma("unroll") for (int u = 0; u < U; ++u) if ((I0) + u < n)                                      \
    {                                                                                                    \
        const v2q *p_ = base + (u64)order[(I0) + u] * stride;                                            \
        DST[u] = NT ? __builtin_nontemporal_load(p_) : *p_;                                              \
    }
        v2q x[U], y[U];
#pragma unroll
        for (int u = 0; u < U; ++u) x[u] = y[u] = v2q{0, 0};
        UTM_GROUP_LOAD(x, 0u)
        u64 cov0 = 0, cov1 = 0;
        for (unsigned i = 0; i < n; i += U) {
            if (i + U < n) { UTM_GROUP_LOAD(y, i + U) }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (i + u < n) {  // (uniform)
                    const u64 newly0 = group_newly(x[u].x, cov0), newly1 = group_newly(x[u].y, cov1);
                    if (newly0 | newly1) group_add<PRIV>(newly0, newly1, mk, stride, G, i + u, n, R, head, bins);
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) x[u] = y[u];
        }
#undef UTM_GROUP_LOAD
    }
    __syncthreads();
    for (unsigned q = threadIdx.x; q < n_head; q += 256)
        if (head[q]) __hip_atomic_fetch_add(&bins[(u64)(q / R) * n + q % R], (u64)head[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
