// Stand-alone check of the integer loop's compaction policy and of the copy's size arithmetic (utmos_amd/csrc/compact_policy.h)
// for a sanitizer build; pure host code, no GPU call:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -I utmos_amd/csrc tools/compact_host_check.cpp -o compact_host_check && ./compact_host_check
// Thresholds at equality, the V_min edges, the batch schedule summing to any k_max, kept = 0 and kept = n_var.
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

int main()
{
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
