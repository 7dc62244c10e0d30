// Stand-alone check of the integer loop's compaction policy and of the copy's size arithmetic (utmos_amd/csrc/compact_policy.h)
// for a sanitizer build; pure host code, no GPU call:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -I utmos_amd/csrc tools/compact_host_check.cpp -o compact_host_check && ./compact_host_check
// Thresholds at equality, the V_min edges, the batch schedule summing to any k_max, kept = 0 and kept = n_var; the
// library's policy by cost swept over V_work, uncovered, the selectable samples and the iterations around every batch
// end (nothing overflows, nothing is compacted that would drop nothing), and the explicit settings against a copy of the
// expression they replaced.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "compact_policy.h"

static long checked = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        ++checked;                                                         \
        if (!(cond)) {                                                     \
            fprintf(stderr, "%s:%d: %s does not hold\n", __FILE__, __LINE__, #cond); \
            return 1;                                                      \
        }                                                                  \
    } while (0)

// The policy as it was before the rule by cost: what explicit settings must still decide, bit for bit.
static CompactDecision old_policy(uint64_t v_work, uint64_t uncovered, uint64_t v_min, double ratio, int64_t iter)
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

// V_work from 0 to 2^40, uncovered from 0 to V_work, A from 0 to 2^20, iterations at and around every batch end.
static int sweep_rules()
{
    std::vector<uint64_t> vs{0, 1, 2, 63, 64, 65, 8191, 8192, 8193, 1000000, UTM_COMPACT_MIN_VARS - 1, UTM_COMPACT_MIN_VARS, UTM_COMPACT_MIN_VARS + 1, 10000000};
    for (int b = 22; b <= 40; b += 3) {
        vs.push_back((1ull << b) - 1);
        vs.push_back(1ull << b);
    }
    const std::vector<uint64_t> as{0, 1, 2, 37, 500, 2008, 2504, 65535, 65536, (1ull << 20) - 1, 1ull << 20};
    std::vector<int64_t> iters{-1, 0, 1};
    for (int64_t e : {16, 48, 112, 240, 496, 752, 1008, 2504})
        for (int64_t d = -1; d <= 1; ++d) iters.push_back(e + d);
    for (uint64_t v : vs) {
        std::vector<uint64_t> us{0, 1, v / 1000, v / 8, v / 2, v / 2 + 1, v - v / 8, v - (v ? 1 : 0), v};
        for (uint64_t u : us) {
            if (u > v) continue;
            for (int64_t iter : iters) {
                // explicit settings: today's decisions exactly, whatever the two new arguments say
                for (uint64_t v_min : std::vector<uint64_t>{1, 64, UTM_COMPACT_MIN_VARS, 1ull << 30})
                    for (double ratio : {0.001, 0.35, 0.5, 0.7, 0.99}) {
                        const CompactDecision was = old_policy(v, u, v_min, ratio, iter);
                        for (uint64_t a : {(uint64_t)0, (uint64_t)2504, (uint64_t)1 << 20}) {
                            const CompactDecision now = compact_policy(v, u, v_min, ratio, iter, a, compact_wp(v));
                            CHECK(now.compact == was.compact && now.batch == was.batch);
                        }
                        const CompactDecision now = compact_policy(v, u, v_min, ratio, iter);
                        CHECK(now.compact == was.compact && now.batch == was.batch);
                    }
                // the library's policy
                for (uint64_t a : as) {
                    const uint64_t wp = compact_wp(v);
                    const CompactDecision d = compact_policy(v, u, 0, 0.0, iter, a, wp);
                    CHECK(d.batch >= 1 && d.batch <= UTM_COMPACT_BATCH);
                    if (u == v || v == 0 || a == 0) CHECK(!d.compact);  // nothing would be dropped / nothing is streamed
                    // the size rule in 128-bit arithmetic: the saturating product decides the same
                    const unsigned __int128 per_iter = (unsigned __int128)a * wp * 8;
                    const bool streams = per_iter > UTM_COMPACT_STREAM_BYTES;
                    if (!streams) CHECK(!d.compact && d.batch == UTM_COMPACT_BATCH);
                    if (streams && v) CHECK(d.batch == old_policy(v, u, 1, 0.5, iter).batch);
                    if (streams && u < v) {
                        // the saving rule in 128-bit integers (8 x the bytes, the cost as 3 / 1), away from equality
                        const unsigned __int128 wasted = (unsigned __int128)(v - u) * a * (unsigned)d.batch;
                        const unsigned __int128 pass = (unsigned __int128)(v + u) * a;
                        const double cost = UTM_COMPACT_PASS_COST;
                        if ((double)wasted > cost * (double)pass * 1.000001) CHECK(d.compact);
                        if ((double)wasted < cost * (double)pass * 0.999999) CHECK(!d.compact);
                    }
                    // a caller that wants fewer iterations than the batch: those decide, the batch stays the schedule's;
                    // more than the batch changes nothing
                    for (int64_t left : {(int64_t)1, (int64_t)4, (int64_t)d.batch, (int64_t)d.batch + 1, (int64_t)1 << 40}) {
                        const CompactDecision l = compact_policy(v, u, 0, 0.0, iter, a, wp, left);
                        CHECK(l.batch == d.batch);
                        if (left >= d.batch) CHECK(l.compact == d.compact);
                        if (l.compact) CHECK(d.compact);
                        if (left <= 3) CHECK(!l.compact);  // (cost 3: three reads never repay a pass)
                    }
                    // monotone in `uncovered`: a lower bound that fails the rule means the true count fails it too
                    if (u && !compact_policy(v, u - 1, 0, 0.0, iter, a, wp).compact) CHECK(!d.compact);
                }
            }
        }
    }
    CHECK(compact_sat_mul(0, UINT64_MAX) == 0 && compact_sat_mul(UINT64_MAX, 2) == UINT64_MAX && compact_sat_mul(1ull << 32, 1ull << 31) == 1ull << 63 &&
          compact_sat_mul(1ull << 32, 1ull << 32) == UINT64_MAX);
    // the shapes the threshold is there for: 2M x 500 (125 MB) is left alone, 10M x 2,504 and 1.1M x 2,504 are not
    CHECK(!compact_policy(2000000, 100000, 0, 0.0, 16, 500, compact_wp(2000000)).compact);
    CHECK(compact_policy(2000000, 100000, 0, 0.0, 16, 500, compact_wp(2000000)).batch == UTM_COMPACT_BATCH);
    CHECK(compact_policy(10000000, 5840000, 0, 0.0, 16, 2488, compact_wp(10000000)).compact);
    CHECK(compact_policy(1103547, 640000, 0, 0.0, 16, 2488, compact_wp(1103547)).compact);
    // one rank's share of 50M x 12,500 asked for 20 iterations: four are left at iteration 16, no copy
    CHECK(compact_policy(50000000, 32000000, 0, 0.0, 16, 12484, compact_wp(50000000)).compact);
    CHECK(!compact_policy(50000000, 32000000, 0, 0.0, 16, 12484, compact_wp(50000000), 4).compact);
    return 0;
}

int main()
{
    if (sweep_rules()) return 1;
    const uint64_t v_min = UTM_COMPACT_MIN_VARS;
    // thresholds at equality: uncovered == ratio x V compacts, one more variant does not
    for (uint64_t v : std::vector<uint64_t>{v_min, v_min + 1, 3 * v_min + 7, 10000000, (1ull << 40) - 1}) {
        for (double ratio : {0.5, 0.25, 0.99, 0.001}) {
            const uint64_t at = (uint64_t)((double)v * ratio);  // floor: the largest count with uncovered <= ratio x V
            CHECK(compact_policy(v, at, v_min, ratio, 300).compact == (at < v));
            CHECK(!compact_policy(v, at + 1, v_min, ratio, 300).compact || (double)(at + 1) <= (double)v * ratio);
            CHECK(compact_policy(v, 0, v_min, ratio, 300).compact);
            CHECK(!compact_policy(v, v, v_min, ratio, 300).compact);  // a copy that drops nothing is never made
        }
        CHECK(compact_policy(v, v / 2, v_min, 0.5, 0).compact);
        CHECK(!compact_policy(v, v / 2 + 1, v_min, 0.5, 0).compact);
    }
    // V_min edges: one variant short of it is left alone, whatever is covered, and runs the usual batches
    CHECK(!compact_policy(v_min - 1, 0, v_min, 0.5, 0).compact);
    CHECK(compact_policy(v_min - 1, 0, v_min, 0.5, 0).batch == UTM_COMPACT_BATCH);
    CHECK(compact_policy(v_min, v_min / 2, v_min, 0.5, 0).compact);
    CHECK(compact_policy(v_min, v_min / 2, v_min, 0.5, 0).batch == 16);
    CHECK(compact_policy(1, 0, 1, 0.5, 0).compact && !compact_policy(0, 0, 1, 0.5, 0).compact && !compact_policy(0, 0, 0, 0.5, 0).compact);
    CHECK(!compact_policy(1, 1, 1, 0.99, 0).compact);
    // the batch schedule: 16, 32, 64, 128, then 256s; from any start it lands on the same boundaries, and cut at k_max the
    // batches sum to k_max
    {
        const int want[] = {16, 32, 64, 128, 256, 256};
        int64_t iter = 0;
        for (int b : want) {
            CHECK(compact_policy(v_min, v_min, v_min, 0.5, iter).batch == b);
            iter += b;
        }
    }
    for (int64_t start = 0; start <= 600; ++start)
        for (int64_t k_max : std::vector<int64_t>{1, 2, 3, 15, 16, 17, 47, 48, 49, 240, 241, 255, 256, 257, 2504}) {
            int64_t iter = start, enq = 0;
            int batches = 0;
            while (enq < k_max) {
                const int b = compact_policy(v_min, v_min, v_min, 0.5, iter).batch;
                CHECK(b >= 1 && b <= UTM_COMPACT_BATCH);
                const int64_t n = b < k_max - enq ? b : k_max - enq;
                if (n == b && iter < 240) CHECK(iter + n == 16 || iter + n == 48 || iter + n == 112 || iter + n == 240);
                iter += n;
                enq += n;
                ++batches;
            }
            CHECK(enq == k_max && iter == start + k_max && batches <= 5 + k_max / UTM_COMPACT_BATCH);
        }
    // the copy: whole KiB per column, at least one; kept = 0 and kept = n_var
    CHECK(compact_wp(0) == 128 && compact_wp(1) == 128 && compact_wp(64 * 128) == 128 && compact_wp(64 * 128 + 1) == 256);
    for (uint64_t n_var : std::vector<uint64_t>{1, 63, 64, 65, 8191, 8192, 8193, 10000000, (1ull << 40) - 1}) {
        const uint64_t wp = compact_wp(n_var);
        CHECK(wp % UTM_COMPACT_WORD_ALIGN == 0 && wp * 64 >= n_var && (wp - UTM_COMPACT_WORD_ALIGN) * 64 < n_var);
        for (uint64_t kept : std::vector<uint64_t>{0, n_var / 2, n_var}) CHECK(compact_wp(kept) <= wp && compact_wp(kept) >= UTM_COMPACT_WORD_ALIGN);
        CHECK(compact_capacity_words(2504, wp) == 2504 * wp);
    }
    CHECK(compact_capacity_words(0, 128) == 0 && compact_capacity_words(1, 128) == 128);
    CHECK(compact_capacity_words(1u << 31, 1ull << 40) == 0);                  // (does not fit a byte count)
    CHECK(compact_capacity_words(3, (UINT64_MAX / 8) / 3) == 3 * ((UINT64_MAX / 8) / 3));
    // exact-size buffers of wp words per column take every kept bit: the last one lands inside
    for (uint64_t kept : std::vector<uint64_t>{1, 64, 65, 8192, 8193, 70001}) {
        std::vector<uint64_t> col(compact_wp(kept), 0);
        col[(kept - 1) >> 6] |= 1ull << ((kept - 1) & 63);
        CHECK(col[(kept - 1) >> 6] != 0);
    }
    printf("compact_host_check: %ld checks ok\n", checked);
    return 0;
}
