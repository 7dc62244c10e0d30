// Coverage bound: a certified upper bound on what ANY panel of k samples can capture (utm_coverage_bound).
#pragma once
#include "common.hip.h"
#include "score_af.hip.h"
#include "swap.hip.h"

// ------------------------------------------------------------------------------------------------
// For multipliers lambda_v in [0, 1], one per live variant, and any k columns S (y_v = 1 when some column of S carries v):
//
//     F(S) = sum_v y_v <= sum_v (1 - lambda_v) y_v + sum_v lambda_v sum_{j in S} a_vj
//                      <= sum_v (1 - lambda_v) + (the k largest column sums s_j = sum_{v in j} lambda_v)   =: L(lambda)
//
// Every lambda gives a bound; projected subgradient steps on L approach the LP bound of maximum coverage.  lambda is kept
// in 16-bit fixed point (Q = 65,536 = 1.0), so every quantity is an integer and the kernels, the CPU build
// (host_bound.hip.h) and the numpy restatement (tests/bound_ref.py) agree bit for bit.  One iteration t:
//
//   k_bound_sums    s_j = sum of lambda over the variants candidate j carries          (one pass over the candidate columns)
//   k_bound_pick    P = the min(k, n_c) positions of the largest s_j, ties to the smaller position (a threshold search);
//                   hist[t] = L_t = sum_live (Q - lambda_v) + sum_{j in P} s_j
//   k_bound_update  c_v = the columns of P that carry v;  lambda_v <- clamp(lambda_v - eta_t (c_v - 1), 0, Q);
//                   the next iteration's sum_live (Q - lambda_v)                        (one pass over the picked columns)
//
// lambda lives in HBM as one uint32 per variant position (wp * 64 per chunk).  A position that is not live -- padding, or a
// variant some `given` sample carries -- holds 0 from k_bound_init on and is never updated: it adds nothing to any s_j, so
// k_bound_sums needs no mask of its own, only lambda.
//
// k_bound_sums follows k_score_aft (score_af.hip.h, read its comment first): a 4,096-variant tile, groups of 4 variants,
// a 16-entry table of the exact partial sums per group, a column nibble is the index.  Here a table value is at most
// 4 Q = 2^18, so an entry is ONE 32-bit word (no limbs, no admission gate), the table is 64 KiB and two workgroups share
// a CU.  Layout: entry (group j of lane sub, nibble b) at word (j * 16 + b) * 32 + sub -- the 32 lanes of a half wave
// (one sample's 32 subs) read 32 different banks whatever their nibbles are.  A lane adds 32 entries per unit and tile:
// at most 2^23.  Its 32-bit partial sum is carried over a run of at most UTM_BOUND_RUN = 16 tiles, so it stays below 2^27,
// and is widened there: the half-wave sum goes in two 16-bit pieces (each piece's 32-lane sum is below 2^21) into one
// 64-bit atomic per sample and run.  Integer addition: the order of the atomics cannot matter.
// ------------------------------------------------------------------------------------------------
#define UTM_BOUND_Q 65536u
#define UTM_BOUND_TILE_WORDS 64  // 4,096 variants = 512 B of a column = 32 lanes x 16 B
#define UTM_BOUND_THREADS 1024
#define UTM_BOUND_MAXU 4         // units (two samples each) a wave keeps in registers over a run: 128 samples per workgroup
#define UTM_BOUND_RUN 16         // tiles between two flushes: a lane's 32-bit sum grows by at most 2^23 per tile
#define UTM_BOUND_GROUP (2 * UTM_BOUND_MAXU * (UTM_BOUND_THREADS / 64))
#define UTM_BOUND_PLANES 17      // k_bound_update counts to 2^17 - 1 and saturates above (see there)
#define UTM_BOUND_PICK_THREADS 1024

// eta_t = max(1, step0 >> min(63, t / period))
UTM_HD unsigned bound_eta(unsigned step0, unsigned period, unsigned t)
{
    const unsigned sh = t / period;
    const unsigned e = sh > 31 ? 0u : step0 >> sh;
    return e ? e : 1u;
}
// lambda <- min(Q, max(0, lambda - eta (c - 1))), c = the picked columns that carry the variant
UTM_HD unsigned bound_step(unsigned lambda, unsigned eta, i64 c)
{
    const i64 x = (i64)lambda - (i64)eta * (c - 1);
    return x < 0 ? 0u : x > (i64)UTM_BOUND_Q ? UTM_BOUND_Q : (unsigned)x;
}

// lambda = Q on the live positions of a chunk, 0 elsewhere (wp * 64 entries, all written); *n_live += popcount(live).
// One thread per 4 positions.
__global__ __launch_bounds__(256) void k_bound_init(const u64 *__restrict__ live, u64 wp, unsigned *__restrict__ lambda, u64 *__restrict__ n_live)
{
    const u64 q = (u64)blockIdx.x * 256 + threadIdx.x;  // 4 positions each
    if (q >= wp * 16) return;
    const u64 word = live[q >> 4];
    const unsigned nib = (unsigned)(word >> ((q & 15) * 4)) & 15u;
    reinterpret_cast<v4u *>(lambda)[q] = v4u{nib & 1 ? UTM_BOUND_Q : 0u, nib & 2 ? UTM_BOUND_Q : 0u, nib & 4 ? UTM_BOUND_Q : 0u, nib & 8 ? UTM_BOUND_Q : 0u};
    if ((q & 15) == 0 && word) atomicAdd(n_live, (u64)__builtin_popcountll(word));
}

// sums[j] += sum of lambda over the set bits of column cand[j] of this chunk.  Grid: (runs of run_tiles tiles) x (groups of
// UTM_BOUND_GROUP candidates); wp is a multiple of 128 words, so every tile lies inside the column as a whole.
__global__ __launch_bounds__(UTM_BOUND_THREADS) void k_bound_sums(const u64 *__restrict__ cols, u64 wp, const unsigned *__restrict__ lambda,
                                                                 const unsigned *__restrict__ cand, unsigned n_cand, u64 *__restrict__ sums,
                                                                 unsigned n_groups, unsigned run_tiles)
{
    constexpr int MAXU = UTM_BOUND_MAXU, NW = UTM_BOUND_THREADS / 64;
    __shared__ __attribute__((aligned(16))) unsigned tab[32 * 16 * 32];  // 64 KiB, layout above
    const unsigned grp = blockIdx.x % n_groups, run = blockIdx.x / n_groups;
    const u64 tiles = wp / UTM_BOUND_TILE_WORDS;
    const u64 t_first = (u64)run * run_tiles;
    if (t_first >= tiles) return;
    const unsigned n_t = (unsigned)(tiles - t_first < run_tiles ? tiles - t_first : run_tiles);
    const unsigned lo = grp * UTM_BOUND_GROUP;
    const unsigned hi = lo + UTM_BOUND_GROUP < n_cand ? lo + UTM_BOUND_GROUP : n_cand;
    if (lo >= hi) return;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const unsigned sub = lane & 31, half = lane >> 5;
    const u64 w_first = t_first * UTM_BOUND_TILE_WORDS;
    // unit u of this wave = positions lo + 2 * (wave + NW * u) + {0, 1}; a lane past the group's ragged end reads the
    // group's last column instead and is cleared before the flush
    const unsigned n_units = (hi - lo + 1) / 2;
    const unsigned n_my = (unsigned)wave < n_units ? (n_units - wave + NW - 1) / NW : 0;  // wave uniform
    const v4u *pa[MAXU];
    unsigned my_s[MAXU];
    bool mine[MAXU];
#pragma unroll
    for (int u = 0; u < MAXU; ++u) {
        const unsigned i = lo + 2 * (wave + NW * u) + half;
        mine[u] = i < hi;
        my_s[u] = cand[mine[u] ? i : hi - 1];
        pa[u] = reinterpret_cast<const v4u *>(cols + (u64)my_s[u] * wp + w_first) + sub;
    }
    // the build: thread (bj, bsub) makes the table of group bj of lane bsub = 4 consecutive lambda values
    const unsigned bj = threadIdx.x >> 5, bsub = threadIdx.x & 31;
    const v4u *lam_thread = reinterpret_cast<const v4u *>(lambda + w_first * 64) + bsub * 32 + bj;
    unsigned *tb_w = tab + bj * 512 + bsub;
    unsigned acc[MAXU];
#pragma unroll
    for (int u = 0; u < MAXU; ++u) acc[u] = 0;
    for (unsigned t = 0; t < n_t; ++t) {
        // this tile's requests go out before the build: they are in flight while the table is made
        v4u x[MAXU];
#pragma unroll
        for (int u = 0; u < MAXU; ++u)
            if ((unsigned)u < n_my) x[u] = __builtin_nontemporal_load(pa[u] + (u64)t * (UTM_BOUND_TILE_WORDS / 2));
        const v4u e = lam_thread[(u64)t * (UTM_BOUND_TILE_WORDS * 16)];
        __syncthreads();  // the previous tile's lookups are done
        {
            unsigned tv[16];
            tv[0] = 0; tv[1] = e.x; tv[2] = e.y; tv[3] = e.x + e.y;
            tv[4] = e.z; tv[5] = e.z + e.x; tv[6] = e.z + e.y; tv[7] = e.z + tv[3];
#pragma unroll
            for (int b = 0; b < 8; ++b) tv[8 + b] = e.w + tv[b];
#pragma unroll
            for (int b = 0; b < 16; ++b) tb_w[b * 32] = tv[b];
        }
        __syncthreads();  // the tables stand
#pragma unroll
        for (int u = 0; u < MAXU; ++u) {
            if ((unsigned)u >= n_my) break;  // wave uniform
            unsigned a = acc[u];
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                const unsigned y = x[u][d];
#pragma unroll
                for (int k = 0; k < 8; ++k) a += tab[((d * 8 + k) * 16 + ((y >> (4 * k)) & 15u)) * 32 + sub];
            }
            acc[u] = a;
        }
        if ((t + 1) % UTM_BOUND_RUN != 0 && t + 1 != n_t) continue;
        // widen: a lane's sum is below 2^27 here; the half wave's goes in two 16-bit pieces
#pragma unroll
        for (int u = 0; u < MAXU; ++u) {
            if ((unsigned)u >= n_my) break;  // wave uniform
            const unsigned a = mine[u] ? acc[u] : 0u;
            acc[u] = 0;
            const unsigned p0 = half_sum32(a & 0xFFFFu), p1 = half_sum32(a >> 16);
            const u64 total = ((u64)p1 << 16) + p0;
            if (sub == 31 && mine[u] && total) atomicAdd(&sums[lo + 2 * (wave + NW * u) + half], total);
        }
    }
}

// One workgroup.  The top kk of the n_cand sums by a threshold search, not a sort: T = the kk-th largest sum is built bit by
// bit from the top bit of the largest sum down (T |= bit while at least kk sums are >= T | bit), one count over the sums and
// one barrier per bit.  Every sum above T is picked, and of the sums equal to T the first kk - count(s > T) in list order
// (a prefix count over the positions: wave ballots, wave totals through LDS, a running base across the blocks of
// positions) -- the tie rule.  The order of picked[] does not matter to anyone (k_bound_update counts, L_t adds), so a slot
// comes from an LDS counter.  Up to UTM_BOUND_PICK_OWN sums per thread stay in registers; with more candidates than that
// every count re-reads them (from L2), so n_cand is not bounded by the workgroup.  A first form ranked every sum by
// counting the sums above it, n_cand^2 / 1024 compares per thread: 0.69 ms at 2,504 candidates, half of the iteration.
// hist[t] = konst[t & 1] + the picked sums; konst[(t + 1) & 1] = 0 for k_bound_update's atomics, and the sums are cleared
// for the next k_bound_sums.
#define UTM_BOUND_PICK_OWN 4
__global__ __launch_bounds__(UTM_BOUND_PICK_THREADS) void k_bound_pick(u64 *__restrict__ sums, const unsigned *__restrict__ cand, unsigned n_cand, unsigned kk,
                                                                      unsigned *__restrict__ picked, u64 *__restrict__ konst, i64 *__restrict__ hist,
                                                                      unsigned t)
{
    constexpr unsigned W = UTM_BOUND_PICK_THREADS, NW = W / 64, OWN = UTM_BOUND_PICK_OWN;
    __shared__ unsigned s_cnt[3];     // the counts of three consecutive passes, used in turn (cleared one pass ahead)
    __shared__ u64 s_max[NW], s_part[NW];
    __shared__ unsigned s_eq[NW], s_slot;
    const unsigned tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const bool small = n_cand <= OWN * W;  // block uniform
    u64 own[OWN];
#pragma unroll
    for (unsigned m = 0; m < OWN; ++m) own[m] = small && tid + m * W < n_cand ? sums[tid + m * W] : 0ull;
    // the workgroup's count of the sums s with s >= lo (ge) or s > lo (!ge); pass = a running number for s_cnt's rotation
    unsigned pass = 0;
    auto count = [&](u64 lo, bool ge) -> unsigned {
        unsigned c = 0;
        if (small) {
#pragma unroll
            for (unsigned m = 0; m < OWN; ++m) c += (tid + m * W < n_cand && (ge ? own[m] >= lo : own[m] > lo)) ? 1u : 0u;
        } else {
            for (unsigned j = tid; j < n_cand; j += W) {
                const u64 v = sums[j];
                c += (ge ? v >= lo : v > lo) ? 1u : 0u;
            }
        }
        c = wave_sum_u32(c);
        if (lane == 0 && c) atomicAdd(&s_cnt[pass % 3], c);
        if (tid == 0) s_cnt[(pass + 1) % 3] = 0;  // (nobody reads or adds to that one between the last barrier and the next)
        __syncthreads();
        const unsigned total = s_cnt[pass % 3];
        ++pass;
        return total;
    };
    // the largest sum: where the search starts
    {
        u64 mx = 0;
        if (small) {
#pragma unroll
            for (unsigned m = 0; m < OWN; ++m) mx = own[m] > mx ? own[m] : mx;
        } else {
            for (unsigned j = tid; j < n_cand; j += W) mx = sums[j] > mx ? sums[j] : mx;
        }
        for (int off = 32; off; off >>= 1) {
            const u64 o = (u64)__shfl_xor((unsigned long long)mx, off, 64);
            mx = o > mx ? o : mx;
        }
        if (lane == 0) s_max[wave] = mx;
        if (tid == 0) s_cnt[0] = s_cnt[1] = s_cnt[2] = 0, s_slot = 0;
        __syncthreads();
    }
    u64 top = 0;
    for (unsigned w = 0; w < NW; ++w) top = s_max[w] > top ? s_max[w] : top;
    u64 T = 0;
    if (kk > 0)
        for (int bit = top ? 63 - __builtin_clzll(top) : -1; bit >= 0; --bit)  // (block uniform)
            if (count(T | (1ull << bit), true) >= kk) T |= 1ull << bit;
    const unsigned above = kk > 0 ? count(T, false) : 0;
    const unsigned need = kk - above;  // of the sums equal to T, in list order (kk == 0: nothing is picked)
    // the picks, a block of W positions at a time
    u64 own_sum = 0;
    unsigned base = 0;  // the sums equal to T at positions before this block
    auto take = [&](unsigned j, u64 v) {
        const bool eq = j < n_cand && v == T, gt = j < n_cand && v > T;
        const u64 vote = __ballot(eq);
        const unsigned before = (unsigned)__builtin_popcountll(vote & ((1ull << lane) - 1));
        __syncthreads();  // the previous block's readers are done with s_eq
        if (lane == 0) s_eq[wave] = (unsigned)__builtin_popcountll(vote);
        __syncthreads();
        unsigned ahead = base, all = 0;
        for (unsigned w = 0; w < NW; ++w) {
            ahead += w < wave ? s_eq[w] : 0u;
            all += s_eq[w];
        }
        base += all;
        if (gt || (eq && ahead + before < need)) {
            picked[atomicAdd(&s_slot, 1u)] = cand[j];
            own_sum += v;
        }
    };
    if (kk > 0 && small) {
#pragma unroll
        for (unsigned m = 0; m < OWN; ++m)
            if (m * W < n_cand) take(m * W + tid, own[m]);  // (block uniform)
    } else if (kk > 0) {
        for (unsigned j0 = 0; j0 < n_cand; j0 += W) take(j0 + tid, j0 + tid < n_cand ? sums[j0 + tid] : 0ull);
    }
    const i64 ws = wave_sum_u63(own_sum);  // (a lane's share is below 2^63: the whole of L_t is)
    if (lane == 0) s_part[wave] = (u64)ws;
    __syncthreads();  // ... and every read of sums[] is done
    for (unsigned j = tid; j < n_cand; j += W) sums[j] = 0;
    if (tid == 0) {
        u64 total = konst[t & 1];
        for (unsigned w = 0; w < NW; ++w) total += s_part[w];
        hist[t] = (i64)total;
        konst[(t + 1) & 1] = 0;
    }
}

// One pass over the kk picked columns of a chunk.  A lane owns a 64-variant word and adds the picked columns' words into
// vertical bit-plane counters with a ripple adder (as depth.hip.h): plane p holds bit p of every variant's count.
// UTM_BOUND_PLANES = 17 planes count to 131,071; a carry out of the last plane is kept as a sticky bit and decoded as
// 131,072.  That is exact: with c - 1 >= Q and eta >= 1 the update gives max(0, lambda - eta (c - 1)) = 0 whatever c is.
// The wave then turns its 64 words around through LDS: lane l takes bit l of every word in turn, so the lambda accesses
// are 256 contiguous bytes per wave instruction.  Every live variant gets the clamp update; sum (Q - lambda') over them is
// at most 64 * 2^16 per lane, its wave sum goes into *konst_next with one atomic per wave.
__global__ __launch_bounds__(256) void k_bound_update(const u64 *__restrict__ cols, u64 wp, const u64 *__restrict__ live, const unsigned *__restrict__ picked,
                                                      unsigned kk, unsigned eta, unsigned *__restrict__ lambda, u64 *__restrict__ konst_next)
{
    constexpr int NP = UTM_BOUND_PLANES;
    __shared__ u64 pl[4][NP + 2][64];  // [wave][plane, sticky, live][word]
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const u64 w0 = (u64)blockIdx.x * 256 + (u64)wave * 64;
    const bool own = w0 < wp;  // (wp is a multiple of 128: a wave's 64 words lie inside the column or past it as a whole)
    const u64 w = own ? w0 + lane : 0;
    const u64 lv = own ? live[w] : 0ull;
    if (!own) kk = 0;
    u64 plane[NP], sticky = 0;
#pragma unroll
    for (int p = 0; p < NP; ++p) plane[p] = 0;
    const u64 *base = cols + w;
    for (unsigned i = 0; i < kk; ++i) {
        u64 carry = base[(u64)picked[i] * wp] & lv;
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            if (__ballot(carry != 0) == 0) break;  // wave uniform
            const u64 up = plane[p] & carry;
            plane[p] ^= carry;
            carry = up;
        }
        sticky |= carry;
    }
    // planes in use: bit_length(kk), at most NP (wave uniform)
    int np = 0;
    while (np < NP && (kk >> np) != 0) ++np;
#pragma unroll
    for (int p = 0; p < NP; ++p) pl[wave][p][lane] = plane[p];
    pl[wave][NP][lane] = sticky;
    pl[wave][NP + 1][lane] = lv;
    __syncthreads();  // (a wave reads only its own rows; a wave past the column's end holds zeros and updates nothing)
    unsigned slack = 0;
    unsigned *lam = lambda + w0 * 64 + lane;
    for (int i = 0; i < 64; ++i) {
        if (pl[wave][NP + 1][i] == 0) continue;  // wave uniform: nothing live in this word
        if (!((pl[wave][NP + 1][i] >> lane) & 1)) continue;
        i64 c = 0;
        for (int p = 0; p < np; ++p) c |= (i64)((pl[wave][p][i] >> lane) & 1) << p;
        if ((pl[wave][NP][i] >> lane) & 1) c = (i64)1 << NP;
        const unsigned l1 = bound_step(lam[i * 64], eta, c);
        lam[i * 64] = l1;
        slack += UTM_BOUND_Q - l1;
    }
    const unsigned s0 = wave_sum_u32(slack & 0xFFFFu), s1 = wave_sum_u32(slack >> 16);  // (a lane: at most 2^22)
    const u64 total = ((u64)s1 << 16) + s0;
    if (lane == 0 && total) atomicAdd(konst_next, total);
}
