// Stand-alone check of the integer loop's list policy, tile rule, launch shape and offset scan (utmos_amd/csrc/list_policy.h)
// for a sanitizer build; pure host code, no GPU call:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -I utmos_amd/csrc tools/list_host_check.cpp -o list_host_check && ./list_host_check
// The gate at equality and on either side of the byte floor, the two shapes the suite binds to the bitmap path, the tile
// rule over every column length up to 2^26 words and at the arrival field's limit, launch shapes of both forms (whole
// rounds, every position covered, workgroups within the target, saturation), the lanes rule at its threshold and on the
// headline shape's six builds, and the scan against a plain recount (padding, empty segments, the 32-bit limit).
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
    // launch shapes: groups of whole rounds (4 positions a round at 64 lanes, 16 at 16) that cover every position and keep
    // the workgroups within the target plus rounding
    for (uint64_t round : {4ull, 16ull})
        for (uint64_t target : {1ull, 64ull, 1024ull, 2048ull, 4096ull, 65536ull})
            for (uint64_t a = 1; a <= 70000; a += (a < 3000 ? 1 : 997))
                for (uint64_t tiles : {1ull, 2ull, 5ull, 23ull, 48ull, 4095ull}) {
                    const uint64_t g = list_group(a, tiles, round, target);
                    const uint64_t groups = (a + g - 1) / g;
                    CHECK(g >= round && g % round == 0 && groups * g >= a && (groups - 1) * g < a);
                    CHECK(groups * tiles <= target + tiles || g == round);
                }
    // ... the whole-wave form's as they were: ceil(a x tiles / 1,024) rounded up to 4
    for (uint64_t a = 1; a <= 3000; ++a)
        for (uint64_t tiles : {1ull, 14ull, 23ull, 38ull, 48ull}) {
            uint64_t g = (a * tiles + UTM_LIST_TARGET_WGS - 1) / UTM_LIST_TARGET_WGS;
            g = (g + 3) / 4 * 4;
            CHECK(list_group(a, tiles, 4, list_target_wgs(64, 0)) == (g < 4 ? 4 : g));
            CHECK(list_group(a, tiles, 4, list_target_wgs(64, 4096)) == (g < 4 ? 4 : g));  // (a forced target is the row form's)
        }
    CHECK(list_target_wgs(16, 0) == UTM_LIST_TARGET_WGS_ROWS && list_target_wgs(16, 64) == 64 && list_target_wgs(64, 0) == UTM_LIST_TARGET_WGS);
    // ... and absurd inputs saturate: no wrap to a small group, no division by zero
    CHECK(list_group(UINT64_MAX, UINT64_MAX, 4, 1024) >= UINT64_MAX / 1024 && list_group(UINT64_MAX, UINT64_MAX, 4, 1024) % 4 == 0);
    CHECK(list_group(UINT64_MAX, UINT64_MAX, 16, 1) == UINT64_MAX);  // (saturated)
    CHECK(list_group(UINT64_MAX, 1, 16, UINT64_MAX) == 16 && list_group(0, 0, 16, 2048) == 16 && list_group(5, 5, 0, 0) == 28);
    // lanes per segment: the mean segment against one batch of a row, at equality and one past it
    CHECK(list_lanes(64 * 10, 2, 5) == 16 && list_lanes(64 * 10 + 1, 2, 5) == 64 && list_lanes(0, 2, 5) == 16);
    CHECK(list_lanes(0, 0, 5) == 64 && list_lanes(7, 3, 0) == 64);  // (no segment at all: the form there has always been)
    CHECK(list_lanes(UINT64_MAX, UINT64_MAX, UINT64_MAX) == 16 && list_lanes(UINT64_MAX, 1, 1) == 64 && list_lanes(1, UINT64_MAX, UINT64_MAX) == 16);
    for (uint64_t tiles = 1; tiles <= 48; ++tiles)
        for (uint64_t listed = 1; listed <= 2504; listed += 9)
            for (uint64_t mean : {1ull, 63ull, 64ull, 65ull, 1000ull}) {
                const uint64_t q = mean * tiles * listed;
                CHECK(list_lanes(q, tiles, listed) == (mean <= UTM_LIST_ROW_QUADS ? 16 : 64));
                CHECK(list_lanes(q + 1, tiles, listed) == (mean < UTM_LIST_ROW_QUADS ? 16 : 64));
            }
    // ... and only the tiles that have the 16-lane form take it
    for (int t : {0, 13, 14, 16, 18, 20})
        for (int l : {0, 16, 64, 7}) CHECK(list_lanes_of_tile(t, l) == ((l == 16 && (t == 13 || t == 16)) ? 16 : 64));
    // the six builds of the headline shape (10M x 2,504, select all: padded entries / 4, tiles, listed columns)
    {
        const uint64_t b[6][3] = {{178723988 / 4, 23, 2488}, {62179312 / 4, 18, 2456}, {26677104 / 4, 14, 2392},
                                  {11939040 / 4, 38, 2264},  {4907380 / 4, 24, 2008},  {2606020 / 4, 16, 1752}};
        const int want[6] = {64, 64, 64, 16, 16, 16};
        for (int k = 0; k < 6; ++k) CHECK(list_lanes(b[k][0], b[k][1], b[k][2]) == want[k]);
        // ... whose 16-lane launches leave a wave 3, 2 and 1 rounds at the default target
        CHECK(list_group(2264, 38, 16, list_target_wgs(16, 0)) == 48 && list_group(2008, 24, 16, list_target_wgs(16, 0)) == 32 &&
              list_group(1752, 16, 16, list_target_wgs(16, 0)) == 16);
    }
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
