// Integer scores from per-sample entry lists: the build kernels and k_score_list.
//
// A list view belongs to one generation of a chunk's working view (host_list.hip.h).  The view's variant axis is cut into
// tiles of 2^T positions; for every (tile, listed column) there is one segment of tile-local u32 entries -- the set bits of
// the column in that tile, ascending -- padded to whole quads of 4 with the sentinel 2^T, which indexes one extra word
// behind the tile's live mask that is always zero.  seg_off[tile * stride + sample] is the segment's first quad, the next
// table entry its end (the table is one exclusive scan, tile-major); unlisted columns have empty segments.  A column is
// immutable, so a list stays right for as long as its view lives: what dies is the mask bit an entry points at.
#pragma once
#include "common.hip.h"
#include "pick.hip.h"
#include "score_int.hip.h"

// counts[tile * stride + s] = set bits of listed column s in the tile.  Grid = tiles x column groups, one wave per piece.
__global__ __launch_bounds__(256) void k_list_count(const u64 *__restrict__ cols, u64 wp, unsigned tile_words, const unsigned *__restrict__ list,
                                                    unsigned n_list, unsigned stride, unsigned *__restrict__ counts)
{
    const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const u64 w0 = (u64)blockIdx.x * tile_words;
    if (w0 >= wp) return;
    const u64 left = wp - w0;
    const unsigned nw2 = (unsigned)(left < tile_words ? left : tile_words) / 2;  // (wp and the tile are whole KiB)
    for (unsigned j = blockIdx.y * 4 + wave; j < n_list; j += gridDim.y * 4) {
        const unsigned s = list[j];
        const v2q *p = reinterpret_cast<const v2q *>(cols + (u64)s * wp + w0);
        unsigned n = 0;
        for (unsigned k = lane; k < nw2; k += 64) {
            const v2q x = p[k];
            n += __popcll(x.x) + __popcll(x.y);
        }
        n = wave_sum_u32(n);
        if (lane == 0) counts[(u64)blockIdx.x * stride + s] = n;
    }
}

// The entries of every (tile, listed column) piece, at the offsets the scan of the counts gave.  One wave per piece, 64
// words a round: a lane's rank is the prefix popcount over the lanes before it plus the rounds before, so entries come
// out ascending and no two lanes share a slot -- plain vector stores, no atomics.  The pad slots get the sentinel.
__global__ __launch_bounds__(256) void k_list_fill(const u64 *__restrict__ cols, u64 wp, unsigned tile_words, const unsigned *__restrict__ list,
                                                   unsigned n_list, unsigned stride, const unsigned *__restrict__ seg_off,
                                                   unsigned *__restrict__ entries)
{
    const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const u64 w0 = (u64)blockIdx.x * tile_words;
    if (w0 >= wp) return;
    const u64 left = wp - w0;
    const unsigned nw = (unsigned)(left < tile_words ? left : tile_words);
    const unsigned sentinel = tile_words * 64;
    for (unsigned j = blockIdx.y * 4 + wave; j < n_list; j += gridDim.y * 4) {
        const unsigned s = list[j];
        const u64 *col = cols + (u64)s * wp + w0;
        const u64 at = (u64)blockIdx.x * stride + s;
        const unsigned q0 = seg_off[at], q1 = seg_off[at + 1];
        unsigned *out = entries + (u64)q0 * 4;
        const unsigned room = (q1 - q0) * 4;
        unsigned run = 0;
        for (unsigned wb = 0; wb < nw; wb += 64) {  // (uniform; nw is a multiple of 128)
            u64 x = col[wb + lane];
            const unsigned n = __popcll(x);
            const unsigned incl = wave_scan_incl_u32(n);
            unsigned o = run + incl - n;
            const unsigned bit0 = (wb + lane) * 64;
            while (x) {
                const unsigned b = (unsigned)__builtin_ctzll(x);
                x &= x - 1;
                if (o < room) out[o] = bit0 + b;  // (the counts are of these very words: always true)
                ++o;
            }
            run += (unsigned)__builtin_amdgcn_readlane((int)incl, 63);
        }
        if (run + lane < room) out[run + lane] = sentinel;  // (at most 3 pad slots)
    }
}

// ------------------------------------------------------------------------------------------------
// k_score_list: the unit of work, grid, block -> unit map and arrivals of k_score_int, but a sample's piece of a tile is
// its segment of entries instead of its bitmap words.  The workgroup stages ~(covered | pending winner's column) of its
// tile in LDS (group 0 stores the ORed words, as k_score_int does); each wave then streams whole segments with 16-byte
// loads, UTM_LIST_U of them in flight, and for every entry reads one LDS word and tests one bit.  A wave reduction and
// one atomic per (position, tile).  The pick (fused_pick / k_pick) does not know the difference.
//
// L = lanes that share one segment.  64: the form above.  16 (list_score_rows): for builds of short segments a wave takes
// four consecutive positions of act[] per round, one per DPP row of 16 lanes, so a workgroup takes 16; the batch loop runs
// to the longest of the wave's four segments (a row past its end reads the sentinel quad), the reduction stops at the
// row (row_shr 1 / 2 / 4 / 8 leave a row's sum in its lane 15) and lanes 15, 31, 47, 63 issue the four atomics in one
// instruction.  Same layout, same arrivals, same bytes: the host chooses by the build's mean segment (list_lanes).
// ------------------------------------------------------------------------------------------------
#define UTM_LIST_U 4
template <int T>
__device__ __forceinline__ unsigned list_live_bits(const unsigned *live, const v4u e)
{
    return ((live[e.x >> 5] >> (e.x & 31)) & 1u) + ((live[e.y >> 5] >> (e.y & 31)) & 1u) + ((live[e.z >> 5] >> (e.z & 31)) & 1u) +
           ((live[e.w >> 5] >> (e.w & 31)) & 1u);
}

// The row form's loop (L = 16), after the kernel's common head: see k_score_list.  i, s, q0 .. are per lane and equal
// over a row; `ib`, the position of the wave's row 0, is what the wave's control flow goes by.
#define UTM_LIST_ROW_U 4  // 16-byte loads per lane in flight, as UTM_LIST_U: a row's batch is 64 quads
template <int T, int FUSED>
__device__ __forceinline__ void list_score_rows(const v4u *__restrict__ entries, const unsigned *__restrict__ so, unsigned stride,
                                                const unsigned *__restrict__ act, u64 *__restrict__ cnt, const unsigned *live,
                                                unsigned lo, unsigned hi, unsigned ib, unsigned i, unsigned s, unsigned s_next,
                                                unsigned s_next2, unsigned by_pos, const PickArgs &pa, v4u (&x)[UTM_LIST_ROW_U],
                                                unsigned q0, unsigned q1, unsigned nq0, unsigned nq1)
{
    const unsigned r = threadIdx.x & 15;
    const v4u sent4 = {1u << T, 1u << T, 1u << T, 1u << T};
    while (ib < hi) {  // (uniform over the wave: row 0 holds its lowest position)
        unsigned acc = 0;
        if (__builtin_amdgcn_ballot_w64(q0 < q1) != 0) {  // (all four segments empty: nothing but the arrivals)
#pragma unroll
            for (int u = 0; u < UTM_LIST_ROW_U; ++u) acc += list_live_bits<T>(live, x[u]);  // the first batch is in flight already
#pragma unroll 1
            for (unsigned qb = q0 + 16 * UTM_LIST_ROW_U; __builtin_amdgcn_ballot_w64(qb < q1) != 0; qb += 16 * UTM_LIST_ROW_U) {
                // (to the end of the longest of the four segments: a row past its own reads the sentinel quad)
#pragma unroll
                for (int u = 0; u < UTM_LIST_ROW_U; ++u) {
                    const unsigned q = qb + u * 16 + r;
                    x[u] = q < q1 ? entries[q] : sent4;
                }
#pragma unroll
                for (int u = 0; u < UTM_LIST_ROW_U; ++u) acc += list_live_bits<T>(live, x[u]);
            }
        }
        const unsigned done_i = i, done_s = s;
        ib += 16;
        i += 16;
        s = s_next;
        s_next = s_next2;
        q0 = i < hi ? nq0 : 0u;  // (a row at or past hi has no segment: it loads nothing and adds nothing)
        q1 = i < hi ? nq1 : 0u;
        if (ib < hi) {
            // the successor round's first batch, its successor's offsets and the index behind that: before the reduction and the atomics
#pragma unroll
            for (int u = 0; u < UTM_LIST_ROW_U; ++u) {
                const unsigned q = q0 + u * 16 + r;
                x[u] = q < q1 ? entries[q] : sent4;
            }
            if (s_next >= stride) s_next = 0;  // (never: act[] holds local samples; checked here, a round after its load was issued)
            nq0 = so[s_next];
            nq1 = so[s_next + 1];
            s_next2 = i + 32 < hi ? act[i + 32] : 0;
        }
        acc += (unsigned)__builtin_amdgcn_update_dpp(0, (int)acc, 0x111, 0xf, 0xf, true);  // row_shr:1
        acc += (unsigned)__builtin_amdgcn_update_dpp(0, (int)acc, 0x112, 0xf, 0xf, true);  // row_shr:2
        acc += (unsigned)__builtin_amdgcn_update_dpp(0, (int)acc, 0x114, 0xf, 0xf, true);  // row_shr:4
        acc += (unsigned)__builtin_amdgcn_update_dpp(0, (int)acc, 0x118, 0xf, 0xf, true);  // row_shr:8 -> lane 15 of the row
        const bool mine = r == 15 && done_i < hi;
        if (FUSED) {
            const bool drop = pa.test_drop && blockIdx.x == 0 && done_i == lo;  // (test hook: see PickArgs::test_drop)
            if (mine && !drop) atomicAdd(&cnt[done_i], (u64)acc + (1ull << UTM_ARRIVAL_SHIFT));
        } else if (mine && acc) {
            atomicAdd(&cnt[by_pos ? done_i : done_s], (u64)acc);
        }
    }
}

template <int T, int FUSED, int L>
__global__ __launch_bounds__(256) void k_score_list(const v4u *__restrict__ entries, const unsigned *__restrict__ seg_off, unsigned stride,
                                                    const u64 *__restrict__ cols, u64 *__restrict__ covered, u64 wp, const Pending pend,
                                                    const IterState *__restrict__ st, const unsigned *__restrict__ act, u64 *__restrict__ cnt,
                                                    unsigned group_size, unsigned n_groups, unsigned by_pos, const PickArgs pa)
{
    constexpr unsigned TILE_WORDS = (1u << T) / 64;  // u64 words of a column per tile
    constexpr unsigned LIVE_Q = (1u << T) / 128;     // 16-byte pieces of the tile's mask
    __shared__ v4u live4[LIVE_Q + 1];                // ... + the sentinel's word (and three more), always zero
    __shared__ IntCand pick_lds[5];
    const unsigned *live = reinterpret_cast<const unsigned *>(live4);
    static_assert(L == 64 || L == 16, "a segment is shared by a wave or by a DPP row");
    constexpr unsigned STEP = 4 * (64 / L);  // positions of act[] a workgroup takes per round: between a wave's (row's) segments
    static_assert(2 * STEP + 16 <= UTM_PICK_PAD, "the read-ahead of act[] stays inside its padding");
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    unsigned tile, grp;
    const bool has_unit = tile_of_block(wp, TILE_WORDS, n_groups, tile, grp);
    const unsigned lo = grp * group_size;
    const unsigned ib = L == 64 ? lo + wave : lo + wave * 4;  // the wave's (its row 0's) first position
    unsigned i = L == 64 ? ib : ib + (lane >> 4);
    // this wave's first three entries of act[], read ahead of the bounds that say whether they count (act[] is padded and
    // holds sample indices throughout, so the offsets read for them are inside the table too)
    const bool in_act = has_unit && i + 2 * STEP < pa.n_local + UTM_PICK_PAD;
    unsigned s = in_act ? act[i] : 0;
    unsigned s_next = in_act ? act[i + STEP] : 0;
    unsigned s_next2 = in_act ? act[i + 2 * STEP] : 0;
    typedef unsigned v8u __attribute__((ext_vector_type(8)));
    v8u raw;
    asm volatile("s_load_dwordx8 %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=s"(raw) : "s"(st) : "memory");
    const IterHead head = __builtin_bit_cast(IterHead, raw);
    const unsigned n_active = head.n_active;
    if (head.done) return;
    if (FUSED && blockIdx.x == gridDim.x - 1) {
        const unsigned n_tiles = (unsigned)((wp + TILE_WORDS - 1) / TILE_WORDS);
        fused_pick<FUSED>(pa, n_tiles, pick_lds);
        return;
    }
    if (!has_unit) return;
    const u64 w0 = (u64)tile * TILE_WORDS;
    const u64 left = wp - w0;
    const unsigned nq = (unsigned)(left < TILE_WORDS ? left : TILE_WORDS) / 2;  // 16-byte pieces of the mask inside the column
    const unsigned hi = lo + group_size < n_active ? lo + group_size : n_active;
    const unsigned *so = seg_off + (u64)tile * stride;
    if (s >= stride) s = 0;  // (never: act[] holds local samples)
    if (s_next >= stride) s_next = 0;
    if (s_next2 >= stride) s_next2 = 0;
    unsigned q0 = so[s], q1 = so[s + 1];
    unsigned nq0 = so[s_next], nq1 = so[s_next + 1];
    const v4u sent4 = {1u << T, 1u << T, 1u << T, 1u << T};
    v4u x[L == 64 ? UTM_LIST_U : UTM_LIST_ROW_U];
    // the first batch of this wave's first segment is requested before the tile is staged
    if constexpr (L == 64) {
        if (i < hi) {
#pragma unroll
            for (int u = 0; u < UTM_LIST_U; ++u) {
                const unsigned q = q0 + u * 64 + lane;
                x[u] = q < q1 ? entries[q] : sent4;
            }
        }
    } else {
        if (i >= hi) q0 = q1 = 0;  // (a row at or past hi has no segment)
#pragma unroll
        for (int u = 0; u < UTM_LIST_ROW_U; ++u) {  // (a wave past hi asks for nothing: q1 = 0 in all its rows)
            const unsigned q = q0 + u * 16 + (lane & 15);
            x[u] = q < q1 ? entries[q] : sent4;
        }
    }

    v4u *cv = reinterpret_cast<v4u *>(covered + w0);
    const u64 *wcol = pend.fuse ? pending_column(&head, cols, wp, pend) : nullptr;
    const v4u *wc = wcol ? reinterpret_cast<const v4u *>(wcol + w0) : nullptr;
    for (unsigned k = threadIdx.x; k < LIVE_Q + 1; k += 256) {
        v4u c = {~0u, ~0u, ~0u, ~0u};  // behind the column's end, and the sentinel's word: dead
        if (k < nq) {
            c = cv[k];
            if (wc) {
                c |= wc[k];
                // every group of this tile computes the same words; group 0 stores them (see k_score_int)
                if (grp == 0) cv[k] = c;
            }
        }
        live4[k] = ~c;
    }
    __syncthreads();

    if constexpr (L == 16) {
        list_score_rows<T, FUSED>(entries, so, stride, act, cnt, live, lo, hi, ib, i, s, s_next, s_next2, by_pos, pa, x, q0, q1, nq0, nq1);
    } else {
        while (i < hi) {
            unsigned acc = 0;
#pragma unroll 1
            for (unsigned qb = q0; qb < q1; qb += 64 * UTM_LIST_U) {  // (uniform over the wave)
                if (qb != q0) {
#pragma unroll
                    for (int u = 0; u < UTM_LIST_U; ++u) {
                        const unsigned q = qb + u * 64 + lane;
                        x[u] = q < q1 ? entries[q] : sent4;
                    }
                }
#pragma unroll
                for (int u = 0; u < UTM_LIST_U; ++u) acc += list_live_bits<T>(live, x[u]);
            }
            const unsigned done_i = i, done_s = s;
            i += 4;
            s = s_next;
            s_next = s_next2;
            q0 = nq0;
            q1 = nq1;
            if (i < hi) {
                // the successor's first batch, its successor's offsets and the index behind that: before the reduction and the atomic
#pragma unroll
                for (int u = 0; u < UTM_LIST_U; ++u) {
                    const unsigned q = q0 + u * 64 + lane;
                    x[u] = q < q1 ? entries[q] : sent4;
                }
                nq0 = so[s_next];
                nq1 = so[s_next + 1];
                s_next2 = i + 8 < hi ? act[i + 8] : 0;
                if (s_next2 >= stride) s_next2 = 0;
            }
            acc = wave_sum_u32(acc);
            if (FUSED) {
                const bool drop = pa.test_drop && blockIdx.x == 0 && done_i == lo;  // (test hook: see PickArgs::test_drop)
                if (lane == 0 && !drop) atomicAdd(&cnt[done_i], (u64)acc + (1ull << UTM_ARRIVAL_SHIFT));
            } else if (lane == 0 && acc) {
                atomicAdd(&cnt[by_pos ? done_i : done_s], (u64)acc);
            }
        }
    }
}
