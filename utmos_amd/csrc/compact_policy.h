// When the integer loop compacts a chunk's working view, how long its batches are meanwhile, and the sizes of the copy.
// Pure host arithmetic, no HIP: included by utmos_hip.hip and built on its own by tools/compact_host_check.cpp.
#pragma once
#include <stdint.h>

#define UTM_COMPACT_MIN_VARS (1ull << 21)  // explicit settings: the variant count that stands for a min_vars of 0
#define UTM_COMPACT_RATIO 0.5              // explicit settings: the share that stands for a ratio of 0
#define UTM_COMPACT_LOG 16                 // passes of a run kept for utm_get_compaction_stats
#define UTM_COMPACT_BATCH 256              // the integer loop's usual batch
#define UTM_COMPACT_WORD_ALIGN 128         // column length granule, in words (UTM_STEP_WORDS)
// The library's own policy (v_min = 0 below).  A view is compacted again only while one iteration streams more than this
// from it: what the 256 MB Infinity Cache would serve is left alone (the value and the two tests that bind it).
#define UTM_COMPACT_STREAM_BYTES (256ull << 20)
// ... and what a byte of a compaction pass costs in bytes of a scoring launch, in the rule's own bytes (columns in + words
// out; the zero fill, the keep / prefix launches and the pass's host round trip ride on them).  Measured at 10M x 2,504
// against scoring launches at 6.1 TB/s: the chunk-sourced pass at iteration 16 moves them at 1.9 TB/s (3.2), the
// view-sourced ones at 2.3 - 2.75 TB/s (2.7 - 2.2); DESIGN §18.  3 is the upper end.  The rule is flat in it: at a
// 32-iteration batch 3 compacts below 0.83 uncovered, 2 below 0.88, 4 below 0.78.
#define UTM_COMPACT_PASS_COST 3.0

struct CompactDecision {
    bool compact;  // make a new copy at this batch boundary
    int batch;     // iterations to enqueue before the next boundary
};

static inline uint64_t compact_sat_mul(uint64_t a, uint64_t b)
{
    return (a && b > UINT64_MAX / a) ? UINT64_MAX : a * b;
}

// A chunk of v_work working variants (what the loop scores now, wp words per column) of which `uncovered` are left, at
// iteration `iter` of the run, with `a` samples still selectable.  While the chunk can still be compacted the run's first
// batches end at iterations 16, 48, 112 and 240 (16, 32, 64, 128 long from a fresh start): the uncovered share halves
// within the first ~50 picks of a large matrix, and a boundary costs two round trips.  A copy that would drop nothing is
// never made.
//   v_min >= 1 (explicit settings, utm_set_compaction): the chunk can be compacted while v_work >= v_min, and is when at
//     most ratio x v_work are uncovered; `a` and `wp` are not looked at.
//   v_min == 0 (the library's defaults): by cost.  The chunk can be compacted while one iteration streams more than
//     UTM_COMPACT_STREAM_BYTES from it (a x wp x 8), and is when the bytes the next batch would read for nothing exceed
//     the bytes of the pass at UTM_COMPACT_PASS_COST scoring bytes each:
//     (v_work - uncovered) / 8 x a x batch  >  cost x (v_work + uncovered) / 8 x a,
//     `batch` being the next batch or, where the caller wants fewer (`left` > 0: utm_run's k_max less what is enqueued),
//     that many: a run that ends after 20 iterations does not pay at iteration 16 for a copy it reads four times.
//     (Products in double: 2^40 variants x 2^20 samples x 256 stays below 2^69; the size rule saturates.)
static inline CompactDecision compact_policy(uint64_t v_work, uint64_t uncovered, uint64_t v_min, double ratio, int64_t iter, uint64_t a = 0,
                                             uint64_t wp = 0, int64_t left = 0)
{
    CompactDecision d;
    d.compact = false;
    d.batch = UTM_COMPACT_BATCH;
    if (v_work == 0) return d;
    if (v_min ? v_work < v_min : compact_sat_mul(compact_sat_mul(a, wp), 8) <= UTM_COMPACT_STREAM_BYTES) return d;
    const int64_t ends[4] = {16, 48, 112, 240};
    for (int i = 0; i < 4; ++i)
        if (iter < ends[i]) {
            d.batch = (int)(ends[i] - (iter < 0 ? 0 : iter));
            break;
        }
    if (uncovered >= v_work) return d;
    if (v_min) {
        d.compact = (double)uncovered <= (double)v_work * ratio;
    } else {
        const int64_t reads = left > 0 && left < d.batch ? left : d.batch;
        const double wasted = (double)(v_work - uncovered) / 8.0 * (double)a * (double)reads;
        const double pass = ((double)v_work + (double)uncovered) / 8.0 * (double)a;
        d.compact = wasted > UTM_COMPACT_PASS_COST * pass;
    }
    return d;
}

// Words per column of a copy that keeps `kept` variants: whole KiB, at least one (every launch shaped by wp has a grid).
static inline uint64_t compact_wp(uint64_t kept)
{
    const uint64_t w = (kept + 63) / 64;
    const uint64_t wp = (w + UTM_COMPACT_WORD_ALIGN - 1) / UTM_COMPACT_WORD_ALIGN * UTM_COMPACT_WORD_ALIGN;
    return wp ? wp : UTM_COMPACT_WORD_ALIGN;
}

// Words of the copy's column block, or 0 when that does not fit a 64-bit byte count.
static inline uint64_t compact_capacity_words(uint64_t n_cols, uint64_t wp)
{
    if (n_cols && wp > (UINT64_MAX / 8) / n_cols) return 0;
    return n_cols * wp;
}
