// When the integer loop builds per-sample entry lists beside a chunk's working view, the tile of a list and the shape of
// its scoring launches.  Pure host arithmetic, no HIP: included by utmos_hip.hip and built on its own by
// tools/list_host_check.cpp.
#pragma once
#include <stdint.h>

// A list is built only while one iteration of the freshly compacted view streams more than this (selectable samples x
// bytes per column): below it the bitmap launches are served by the Infinity Cache or run as one persistent launch, and two
// tests of the suite bind those paths launch for launch.
#define UTM_LIST_MIN_STREAM_BYTES (1ull << 30)
// ... and only when 4 bytes per entry, c_list times over, still undercut the 8 bytes per word of the bitmap column.
#define UTM_LIST_RATIO 2.0
#define UTM_LIST_LOG 16           // builds of a run kept for utm_get_list_stats
#define UTM_LIST_MAX_TILES 48     // tiles per column the rule aims below: one atomic per (position, tile) on a count word
#define UTM_LIST_TARGET_WGS 1024  // workgroups of a list launch: the device about twice over (256 CUs x 2)
#define UTM_LIST_T_TEST 13        // the smallest tile (8,192 positions = one KiB of a column): tests only
#define UTM_LIST_ROW_QUADS 64     // a build whose mean segment is at most this many quads is scored 16 lanes per segment
#define UTM_LIST_TARGET_WGS_ROWS 2048  // workgroups of such a launch: 8 resident per CU at the 8 KiB mask (256 CUs x 8)
#define UTM_LIST_TARGET_WGS_MAX 65536  // the largest target utm_set_list_shape takes

static inline uint64_t list_sat_mul(uint64_t a, uint64_t b)
{
    return (a && b > UINT64_MAX / a) ? UINT64_MAX : a * b;
}

// Build lists for a view of wp words per column that a compaction pass has just written, `a` columns listed, the previous
// winner having gained `last_new` (< 0: not known).  Greedy gains never rise, so last_new bounds every listed column's
// entry count.  `had_list`: the run has had a list view for this chunk already -- every later pass rebuilds it.
static inline bool list_policy(int64_t last_new, uint64_t wp, uint64_t a, uint64_t min_stream_bytes, double c_list, bool had_list)
{
    if (!wp || !a) return false;
    if (had_list) return true;
    if (last_new < 0) return false;
    if (list_sat_mul(list_sat_mul(a, wp), 8) <= min_stream_bytes) return false;
    return 4.0 * (double)last_new * c_list <= 8.0 * (double)wp;
}

// Tiles of 2^t positions over a column of wp words (wp is a multiple of 128 words = 2^13 positions).
static inline uint64_t list_tiles(uint64_t wp, int t)
{
    const uint64_t tile_words = (1ull << t) / 64;
    return (wp + tile_words - 1) / tile_words;
}

// The tile of a build: the smallest of 2^16, 2^18, 2^20 positions (8, 32, 128 KiB of LDS mask) that cuts the column into
// at most UTM_LIST_MAX_TILES tiles, else the largest; `forced` (tests) is taken as given when it is one of the four sizes
// built.  0: no tile keeps the column within max_tiles (the arrival field of a count word).
static inline int list_tile_log2(uint64_t wp, int forced, uint64_t max_tiles)
{
    int t = 20;
    if (forced == UTM_LIST_T_TEST || forced == 16 || forced == 18 || forced == 20) {
        t = forced;
    } else {
        for (int cand : {16, 18, 20})
            if (list_tiles(wp, cand) <= UTM_LIST_MAX_TILES) { t = cand; break; }
    }
    return list_tiles(wp, t) <= max_tiles ? t : 0;
}

// Lanes of a wave that share one segment in the scoring launches of a build: 64 (a wave walks one segment at a time), or
// 16 (one segment per DPP row, four positions of act[] per wave and round) when the build's mean segment -- `quads` over
// `tiles` x `listed` segments -- is at most UTM_LIST_ROW_QUADS, one batch of a row.  Decided once per build.
static inline int list_lanes(uint64_t quads, uint64_t tiles, uint64_t listed)
{
    const uint64_t segs = list_sat_mul(tiles, listed);
    if (!segs) return 64;
    return quads <= list_sat_mul(segs, UTM_LIST_ROW_QUADS) ? 16 : 64;
}

// The 16-lane form is built for the tiles whose builds have short segments (2^13, 2^16); any other tile keeps 64 lanes,
// whatever the rule or utm_set_list_shape says.
static inline int list_lanes_of_tile(int t, int lanes)
{
    return (lanes == 16 && (t == UTM_LIST_T_TEST || t == 16)) ? 16 : 64;
}

// Positions of act[] per workgroup of a list launch: about `target` workgroups over a x tiles units, in whole rounds of
// `round` positions (4 waves x 64 / lanes: 4 or 16).
static inline uint64_t list_group(uint64_t a, uint64_t tiles, uint64_t round, uint64_t target)
{
    if (!round) round = 4;
    if (!target) target = 1;
    const uint64_t units = list_sat_mul(a, tiles);
    const uint64_t g = units / target + (units % target ? 1 : 0);
    const uint64_t rounds = g / round + (g % round ? 1 : 0);
    return list_sat_mul(rounds ? rounds : 1, round);
}
// ... and the target of a launch: the row form's own, the whole-wave form's as before; `forced` (utm_set_list_shape) > 0
// replaces the row form's.
static inline uint64_t list_target_wgs(int lanes, uint64_t forced)
{
    if (lanes != 16) return UTM_LIST_TARGET_WGS;
    return forced ? forced : UTM_LIST_TARGET_WGS_ROWS;
}

// Exclusive scan of the padded counts (entries rounded up to whole quads of 4), in quads.  counts and offs hold n values
// (+ 1 in offs: the total); per_col[s] += the quads of column s = k % stride.  -> false when an offset would not fit 32 bits.
static inline bool list_scan(const uint32_t *counts, uint64_t n, uint64_t stride, uint32_t *offs, uint32_t *per_col, uint64_t *entries,
                             uint64_t *quads)
{
    uint64_t run = 0, sum = 0;
    for (uint64_t k = 0; k < n; ++k) {
        if (run > UINT32_MAX) return false;
        offs[k] = (uint32_t)run;
        const uint32_t q = counts[k] / 4 + (counts[k] % 4 ? 1 : 0);
        if (per_col && stride) per_col[k % stride] += q;
        run += q;
        sum += counts[k];
    }
    if (run > UINT32_MAX) return false;
    offs[n] = (uint32_t)run;
    *entries = sum;
    *quads = run;
    return true;
}
