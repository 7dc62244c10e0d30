// Stand-alone check of the integer loop's list policy, tile rule, launch shape and offset scan (utmos_amd/csrc/list_policy.h)
// for a sanitizer build; pure host code, no GPU call:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -I utmos_amd/csrc tools/list_host_check.cpp -o list_host_check && ./list_host_check
// The gate at equality and on either side of the byte floor, the two shapes the suite binds to the bitmap path, the tile
// rule over every column length up to 2^26 words and at the arrival field's limit, launch shapes that cover every
// position, and the scan against a plain recount (padding, empty segments, the 32-bit limit).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "list_policy.h"

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
    const uint64_t floor_b = UTM_LIST_MIN_STREAM_BYTES;
    // the gate: 4 x last_new x c <= 8 x wp, at equality and one past it
    CHECK(list_policy(1024, 1024, 2000000, floor_b, 2.0, false));
    CHECK(!list_policy(1025, 1024, 2000000, floor_b, 2.0, false));
    CHECK(!list_policy(-1, 1024, 2000000, floor_b, 2.0, false));
    CHECK(list_policy(-1, 1024, 1, floor_b, 2.0, true));  // a run that has a list rebuilds it
    CHECK(!list_policy(0, 0, 5, 1, 2.0, true) && !list_policy(0, 5, 0, 1, 2.0, true));
    // the byte floor: a x wp x 8 must exceed it
    CHECK(!list_policy(0, 1 << 17, 1024, floor_b, 2.0, false));      // exactly 1 GiB
    CHECK(list_policy(0, (1 << 17) + 128, 1024, floor_b, 2.0, false));
    CHECK(list_policy(0, UINT64_MAX / 2, UINT64_MAX / 2, floor_b, 2.0, false));  // (saturates, no overflow)
    // the shapes the suite keeps on the bitmap path: 1.1M x 2,504 (345 MB) and 2M x 500 (125 MB), whatever is left of them
    for (uint64_t a = 1; a <= 2504; a += 7)
        for (uint64_t wp = 128; wp <= 17280; wp += 128) CHECK(!list_policy(0, wp, a, floor_b, 2.0, false));
    for (uint64_t a = 1; a <= 500; a += 3)
        for (uint64_t wp = 128; wp <= 31360; wp += 128) CHECK(!list_policy(0, wp, a, floor_b, 2.0, false));
    // ... and the headline shape passes it at its first boundaries (10M x 2,504: 730 KB columns after 16 rows)
    CHECK(list_policy(40000, 93440, 2488, floor_b, 2.0, false));
    // the tile rule
    for (uint64_t wp = 128; wp <= (1ull << 26); wp += (wp < 100000 ? 128 : 128 * 977)) {
        const int t = list_tile_log2(wp, 0, 4095);
        CHECK(t == 16 || t == 18 || t == 20 || (t == 0 && list_tiles(wp, 20) > 4095));
        if (t) {
            CHECK(list_tiles(wp, t) * ((1ull << t) / 64) >= wp && (list_tiles(wp, t) - 1) * ((1ull << t) / 64) < wp);
            CHECK(list_tiles(wp, t) <= 4095);
            if (t > 16) CHECK(list_tiles(wp, t - 2) > UTM_LIST_MAX_TILES);
            if (t < 20) CHECK(list_tiles(wp, t) <= UTM_LIST_MAX_TILES);
        }
        for (int f : {13, 16, 18, 20}) {
            const int tf = list_tile_log2(wp, f, 4095);
            CHECK(tf == f || (tf == 0 && list_tiles(wp, f) > 4095));
        }
        CHECK(list_tile_log2(wp, 17, 4095) == t);  // (a size that is not built: the rule's)
    }
    CHECK(list_tiles(128, 13) == 1 && list_tiles(256, 13) == 2 && list_tiles(1024, 16) == 1 && list_tiles(1152, 16) == 2);
    // launch shapes: groups of whole waves' worth that cover every position
    for (uint64_t a = 1; a <= 70000; a += (a < 3000 ? 1 : 997))
        for (uint64_t tiles : {1ull, 2ull, 5ull, 23ull, 48ull, 4095ull}) {
            const uint64_t g = list_group(a, tiles);
            CHECK(g >= 4 && g % 4 == 0 && (a + g - 1) / g * g >= a);
            CHECK((a + g - 1) / g * tiles <= UTM_LIST_TARGET_WGS + tiles || g == 4);
        }
    CHECK(list_group(UINT64_MAX, UINT64_MAX) >= 4);
    // the scan
    uint64_t seed = 12345;
    for (int round = 0; round < 200; ++round) {
        const uint64_t stride = 1 + (uint64_t)round % 17, tiles = 1 + (uint64_t)round % 5, n = stride * tiles;
        std::vector<uint32_t> counts(n), offs(n + 1), per_col(stride, 0);
        for (auto &c : counts) {
            seed = seed * 6364136223846793005ull + 1442695040888963407ull;
            c = (uint32_t)((seed >> 33) % 11);  // 0 .. 10: every padding
        }
        uint64_t entries = 0, quads = 0;
        CHECK(list_scan(counts.data(), n, stride, offs.data(), per_col.data(), &entries, &quads));
        uint64_t run = 0, sum = 0, cols = 0;
        for (uint64_t k = 0; k < n; ++k) {
            CHECK(offs[k] == run);
            run += (counts[k] + 3) / 4;
            sum += counts[k];
        }
        for (auto q : per_col) cols += q;
        CHECK(offs[n] == run && quads == run && entries == sum && cols == run && quads * 4 >= entries && quads * 4 < entries + 4 * n + 1);
    }
    {
        std::vector<uint32_t> counts(3, UINT32_MAX), offs(4);  // 3 x 2^30 quads: the third offset is past 32 bits
        uint64_t entries = 0, quads = 0;
        CHECK(list_scan(counts.data(), 2, 0, offs.data(), nullptr, &entries, &quads) && quads == 2ull << 30);
        counts.assign(5, UINT32_MAX);
        offs.resize(6);
        CHECK(!list_scan(counts.data(), 5, 0, offs.data(), nullptr, &entries, &quads));
    }
    printf("list_host_check: %ld checks hold\n", checked);
    return 0;
}
