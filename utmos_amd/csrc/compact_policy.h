// When the integer loop compacts a chunk's working view, how long its batches are meanwhile, and the sizes of the copy.
// Pure host arithmetic, no HIP: included by utmos_hip.hip and built on its own by tools/compact_host_check.cpp.
#pragma once
#include <stdint.h>

#define UTM_COMPACT_MIN_VARS (1ull << 21)  // a working view shorter than this is never compacted again (why not 2^20)
#define UTM_COMPACT_RATIO 0.5              // compact when at most this share of the working variants is still uncovered
#define UTM_COMPACT_LOG 16                 // passes of a run kept for utm_get_compaction_stats
#define UTM_COMPACT_BATCH 256              // the integer loop's usual batch
#define UTM_COMPACT_WORD_ALIGN 128         // column length granule, in words (UTM_STEP_WORDS)

struct CompactDecision {
    bool compact;  // make a new copy at this batch boundary
    int batch;     // iterations to enqueue before the next boundary
};

// A chunk of v_work working variants (what the loop scores now) of which `uncovered` are left, at iteration `iter` of the
// run.  While the chunk can still be compacted (v_work >= v_min) the run's first batches end at iterations 16, 48, 112
// and 240 (16, 32, 64, 128 long from a fresh start): the uncovered share halves within the first ~50 picks of a large
// matrix, and a boundary costs two round trips.  A copy that would drop nothing is never made.
static inline CompactDecision compact_policy(uint64_t v_work, uint64_t uncovered, uint64_t v_min, double ratio, int64_t iter)
{
    CompactDecision d;
    d.compact = false;
    d.batch = UTM_COMPACT_BATCH;
    if (v_work < v_min || v_work == 0) return d;
    const int64_t ends[4] = {16, 48, 112, 240};
    for (int i = 0; i < 4; ++i)
        if (iter < ends[i]) {
            d.batch = (int)(ends[i] - (iter < 0 ? 0 : iter));
            break;
        }
    d.compact = uncovered < v_work && (double)uncovered <= (double)v_work * ratio;
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
