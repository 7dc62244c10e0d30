// Coverage depth (set multicover): every variant counts until M selected samples carry it (utm_set_depth).
#pragma once
#include "common.hip.h"

// ------------------------------------------------------------------------------------------------
// State: per chunk P = bit_length(M) bit planes of wp words, the word layout of `covered` -- plane p holds bit p of
// every variant's support (the number of selected samples that carry it, saturating at M).  `covered` is the mask
// the scoring kernels read: support == M.  So a scoring pass counts popcount(column & ~covered) = the units a sample
// would add to F = sum_v min(support(v), M), and the kernels of that pass do not change.
//
// k_depth_apply adds ONE column to the planes.  Every 64-variant word is independent of every other: a lane takes 16
// bytes of the column, of covered and of each plane (global_load_dwordx4), ripples the carry through the planes in
// registers and stores covered and the planes back.  Traffic: (2 P + 3) * wp * 8 bytes per chunk.  Two sums come out
// of a launch -- units gained and variants that became saturated: DPP wave sums, the four waves' partials meet in
// LDS, one 64-bit atomic per workgroup and sum (skipped when the partial is 0).
// ------------------------------------------------------------------------------------------------
#define UTM_DEPTH_MAX 255
#define UTM_DEPTH_MAX_PLANES 8

// One word of one column against the word's planes: the whole arithmetic of a depth update, shared with the CPU build
// (utm_depth_apply_host).  cov = the word of `covered` (support == M), pl[p] = the word of plane p.  Only variants
// below M count (add), so the counter never passes M and the carry out of the top plane is always 0.
template <int P>
UTM_HD void depth_word(u64 col, u64 &cov, u64 (&pl)[P], unsigned m, unsigned &units, unsigned &newly)
{
    const u64 add = col & ~cov;
    u64 carry = add;
#pragma unroll
    for (int p = 0; p < P; ++p) {
        const u64 t = pl[p] & carry;
        pl[p] ^= carry;
        carry = t;
    }
    u64 sat = ~0ull;
#pragma unroll
    for (int p = 0; p < P; ++p) sat &= (m >> p & 1u) ? pl[p] : ~pl[p];
    units += (unsigned)__builtin_popcountll(add);
    newly += (unsigned)__builtin_popcountll(sat & ~cov);
    cov = sat;
}

// What a launch inside the loop leaves behind besides the planes: its last workgroup to finish (arrival counter) notes
// the running number of saturated variants for the row just made and takes the winner off the pending state, so that no
// later launch ORs its column into covered.
struct DepthSync {
    unsigned arrived;
    unsigned pad;
};

// col: the column to add, or nullptr = the pending winner of IterState (read on the device, no host read-back).
// sync != nullptr: a launch of the loop (see DepthSync); `commit` is set on the launch of the last chunk.
template <int P>
__global__ __launch_bounds__(256) void k_depth_apply(u64 *__restrict__ covered, u64 *__restrict__ planes, const u64 *__restrict__ cols, u64 wp,
                                                     const Pending pend, IterState *__restrict__ st, const u64 *__restrict__ col, unsigned m,
                                                     u64 *__restrict__ units_out, u64 *__restrict__ sat_out, DepthSync *__restrict__ sync,
                                                     i64 *__restrict__ res_sat, int commit)
{
    __shared__ unsigned part[2][4];
    const u64 *wcol = col ? col : pending_column(st, cols, wp, pend);
    if (!wcol) return;  // (uniform over the grid: the pending state only changes once every workgroup has arrived)
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const u64 n2 = wp / 2;  // 16-byte units of a column (wp is a multiple of UTM_STEP_WORDS)
    const v2q *c2 = reinterpret_cast<const v2q *>(wcol);
    v2q *cv2 = reinterpret_cast<v2q *>(covered);
    unsigned units = 0, newly = 0;
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < n2; i += (u64)gridDim.x * 256) {
        const v2q x = c2[i];
        v2q cv = cv2[i];
        v2q q[P];
#pragma unroll
        for (int p = 0; p < P; ++p) q[p] = reinterpret_cast<const v2q *>(planes + (u64)p * wp)[i];
        u64 a[P], b[P];
#pragma unroll
        for (int p = 0; p < P; ++p) { a[p] = q[p].x; b[p] = q[p].y; }
        u64 cov0 = cv.x, cov1 = cv.y;
        depth_word<P>(x.x, cov0, a, m, units, newly);
        depth_word<P>(x.y, cov1, b, m, units, newly);
        cv2[i] = v2q{cov0, cov1};
#pragma unroll
        for (int p = 0; p < P; ++p) reinterpret_cast<v2q *>(planes + (u64)p * wp)[i] = v2q{a[p], b[p]};
    }
    const unsigned su = wave_sum_u32(units), sn = wave_sum_u32(newly);
    if (lane == 0) { part[0][wave] = su; part[1][wave] = sn; }
    __syncthreads();
    if (threadIdx.x != 0) return;
    const unsigned tu = part[0][0] + part[0][1] + part[0][2] + part[0][3];
    const unsigned tn = part[1][0] + part[1][1] + part[1][2] + part[1][3];
    if (tu) __hip_atomic_fetch_add(units_out, (u64)tu, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (tn) __hip_atomic_fetch_add(sat_out, (u64)tn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (!sync) return;
    // release: this workgroup's sums are out before its arrival; the last one to arrive reads them all (acquire)
    const unsigned before = __hip_atomic_fetch_add(&sync->arrived, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    if (before + 1 != gridDim.x) return;
    __hip_atomic_store(&sync->arrived, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // ready for the next launch
    if (!commit) return;
    res_sat[st->iter - 1] = (i64)__hip_atomic_load(sat_out, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    st->prev_valid = 0;  // nothing stays pending: the next scoring pass is a full one against covered as it now is
}
