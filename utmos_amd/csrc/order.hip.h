// Fixed orders: the coverage curve of a GIVEN list of samples in one streaming pass (utm_apply_order).
#pragma once
#include "common.hip.h"

// ------------------------------------------------------------------------------------------------
// new_count[i] = popcount(col[o_i] & ~(covered | col[o_0] | ... | col[o_{i-1}])) for a list o_0 .. o_{n-1} of columns.
// Every 64-variant word is independent of every other; only the order along the sample axis matters.  So a
// workgroup owns one tile of the variant axis (UTM_ORDER_TILE_WORDS words = 4 KiB: one KiB, i.e. one
// global_load_dwordx4 wave instruction, per wave), keeps the tile's running covered words in registers (16 B per
// lane) and walks the list: gain = w & ~cov, cov |= w, popcount, wave reduction.  The four waves' partials of a
// position meet in LDS; one lane per position adds them and issues ONE 64-bit atomic per (position, tile), skipped
// when the partial is 0 -- and along a coverage curve most partials soon are.  At the end the tile goes back to
// `covered`.  Traffic: n * wp * 8 bytes of columns, `covered` once in and once out.
//
// The walk runs in rounds of UTM_ORDER_U positions: the NEXT round's UTM_ORDER_U KiB per wave are requested before this
// round's reductions, its barrier and its atomics (k_score_int pipelines across samples the same way), so a wave keeps
// 16 KiB in flight.  That depth stands in for occupancy: a column of 10M variants is only 306 tiles = 1,224 waves on
// 1,024 SIMDs, and 1,224 x 16 KiB = 20 MB in flight is what Little's law asks of HBM (a few TB/s x a few us).  A taller
// tile would cut the atomics further but leave CUs without a workgroup; a 1 KiB tile (one wave) would quadruple them.
// The partials are double buffered in LDS: one barrier per round.
// ------------------------------------------------------------------------------------------------
#define UTM_ORDER_TILE_WORDS (4 * UTM_STEP_WORDS)
#define UTM_ORDER_U 16

// One word of one column against the running covered word: the whole arithmetic of the curve, shared with the CPU
// build (utm_order_curve_host).
UTM_HD unsigned order_word(u64 w, u64 &cov)
{
    const u64 gain = w & ~cov;
    cov |= w;
    return (unsigned)__builtin_popcountll(gain);
}

template <bool NT>
__global__ __launch_bounds__(256) void k_order_curve(const u64 *__restrict__ cols, u64 *__restrict__ covered, u64 wp,
                                                     const unsigned *__restrict__ order, unsigned n, u64 *__restrict__ counts)
{
    constexpr int U = UTM_ORDER_U;
    __shared__ unsigned part[2][4][U];  // [round buffer][wave][position - round start]
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const u64 w0 = (u64)blockIdx.x * UTM_ORDER_TILE_WORDS + (u64)wave * UTM_STEP_WORDS;
    // wp is a multiple of UTM_STEP_WORDS: a wave's KiB lies inside the column or past its end as a whole.  A wave past
    // the end (the column's last tile) loads nothing and counts zero, but keeps the barriers.
    const bool own = w0 < wp;
    const v2q *base = reinterpret_cast<const v2q *>(cols + (own ? w0 : 0)) + lane;
    const u64 stride = wp / 2;  // a column, in 16-byte units
#define UTM_ORDER_LOAD(DST, I0)                                                                              \
    if (own) {                                                                                               \
        _Pragma("unroll") for (int u = 0; u < U; ++u) if ((I0) + u < n)                                      \
        {                                                                                                    \
            const v2q *p_ = base + (u64)order[(I0) + u] * stride;                                            \
            DST[u] = NT ? __builtin_nontemporal_load(p_) : *p_;                                              \
        }                                                                                                    \
    }
    v2q x[U], y[U];
#pragma unroll
    for (int u = 0; u < U; ++u) x[u] = y[u] = v2q{0, 0};
    UTM_ORDER_LOAD(x, 0u)
    v2q *cv = reinterpret_cast<v2q *>(covered + (own ? w0 : 0)) + lane;
    v2q cov = own ? *cv : v2q{0, 0};
    u64 cov0 = cov.x, cov1 = cov.y;
    unsigned buf = 0;
    for (unsigned i = 0; i < n; i += U) {
        if (i + U < n) { UTM_ORDER_LOAD(y, i + U) }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (i + u < n) {  // (uniform)
                const unsigned acc = own ? order_word(x[u].x, cov0) + order_word(x[u].y, cov1) : 0u;
                const unsigned sum = wave_sum_u32(acc);
                if (lane == 0) part[buf][wave][u] = sum;
            }
        }
        __syncthreads();  // the round's partials are complete (the other buffer is free again: its readers passed the last barrier)
        if (threadIdx.x < (unsigned)U && i + threadIdx.x < n) {
            const unsigned t = threadIdx.x;
            const unsigned v = part[buf][0][t] + part[buf][1][t] + part[buf][2][t] + part[buf][3][t];
            if (v) atomicAdd(&counts[i + t], (u64)v);
        }
        buf ^= 1;
#pragma unroll
        for (int u = 0; u < U; ++u) x[u] = y[u];
    }
    if (own) *cv = v2q{cov0, cov1};
#undef UTM_ORDER_LOAD
}
