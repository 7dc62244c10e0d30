// Stand-alone check of utm_class_counts_host for a sanitizer build of the HOST code (runs on the CPU, no GPU call):
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -I include \
//         utmos_amd/csrc/utmos_hip.hip tools/class_host_check.cpp -ldl -o class_host_check && ./class_host_check
// A few hundred random shapes -- the sizes of tests/test_classes_host.py and random ones, every class count from 1 to
// UTM_CLASSES_MAX, lists as NULL, a permutation and a strict subset -- with exact-size buffers (so that any access past
// them is caught), against a bit-by-bit loop.  The refusals leave a canary-filled table untouched.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "utmos_hip.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t next64()
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

static int check(uint64_t n_var, uint32_t n_samp, int32_t n_classes, int family, int list_kind)
{
    const uint64_t wp = (n_var + 63) / 64;
    std::vector<uint64_t> cols((size_t)n_samp * wp);
    for (auto &w : cols) w = next64() & next64();
    if (n_var & 63)
        for (uint32_t c = 0; c < n_samp; ++c) cols[(size_t)c * wp + wp - 1] &= (1ull << (n_var & 63)) - 1;
    std::vector<int32_t> class_of((size_t)n_var);
    for (uint64_t v = 0; v < n_var; ++v) {
        switch (family) {
        case 0: class_of[v] = n_classes - 1; break;                                   // one class for all
        case 1: class_of[v] = -1; break;                                              // counted nowhere
        case 2: class_of[v] = n_classes > 1 ? 1 + (int32_t)(next64() % (uint64_t)(n_classes - 1)) : 0; break;  // class 0 empty
        default: class_of[v] = next64() % 10 == 0 ? -1 : (int32_t)(next64() % (uint64_t)n_classes); break;
        }
    }
    std::vector<uint32_t> idx;
    if (list_kind) {  // 1: a permutation, 2: a strict subset of one
        for (uint32_t s = 0; s < n_samp; ++s) idx.push_back(s);
        for (uint32_t s = n_samp; s > 1; --s) std::swap(idx[s - 1], idx[next64() % s]);
        if (list_kind == 2) idx.resize(n_samp > 1 ? n_samp / 2 : 1);
    }
    const size_t rows = list_kind ? idx.size() : n_samp;
    std::vector<int64_t> got(rows * (size_t)n_classes, -77), want(rows * (size_t)n_classes, 0);
    const int rc = utm_class_counts_host(cols.data(), wp, n_var, n_samp, class_of.data(), n_classes, list_kind ? idx.data() : nullptr,
                                         list_kind ? idx.size() : 0, got.data());
    if (rc != UTM_OK) {
        fprintf(stderr, "n_var %llu n_samp %u n_classes %d family %d list %d: rc %d (%s)\n", (unsigned long long)n_var, n_samp, n_classes, family,
                list_kind, rc, utm_last_error());
        return 1;
    }
    for (size_t j = 0; j < rows; ++j) {
        const uint32_t s = list_kind ? idx[j] : (uint32_t)j;
        for (uint64_t v = 0; v < n_var; ++v)
            if ((cols[(size_t)s * wp + (v >> 6)] >> (v & 63) & 1) && class_of[v] >= 0) ++want[j * (size_t)n_classes + (size_t)class_of[v]];
    }
    if (got != want) {
        fprintf(stderr, "n_var %llu n_samp %u n_classes %d family %d list %d: tables differ\n", (unsigned long long)n_var, n_samp, n_classes, family,
                list_kind);
        return 1;
    }
    return 0;
}

static int refusals()
{
    std::vector<uint64_t> cols(4, 0);
    std::vector<int32_t> good(10, 0), bad(10, 0);
    std::vector<int64_t> table(12, -77);
    const uint32_t twice[] = {1, 1}, beyond[] = {0, 4};
    int wrong = 0;
    wrong += utm_class_counts_host(cols.data(), 1, 10, 4, nullptr, 3, nullptr, 0, table.data()) != UTM_EINVAL;
    wrong += utm_class_counts_host(cols.data(), 1, 10, 4, good.data(), 3, nullptr, 0, nullptr) != UTM_EINVAL;
    wrong += utm_class_counts_host(cols.data(), 1, 10, 4, good.data(), 0, nullptr, 0, table.data()) != UTM_EINVAL;
    wrong += utm_class_counts_host(cols.data(), 1, 10, 4, good.data(), UTM_CLASSES_MAX + 1, nullptr, 0, table.data()) != UTM_EINVAL;
    bad[9] = 3;
    wrong += utm_class_counts_host(cols.data(), 1, 10, 4, bad.data(), 3, nullptr, 0, table.data()) != UTM_EINVAL;
    bad[9] = -2;
    wrong += utm_class_counts_host(cols.data(), 1, 10, 4, bad.data(), 3, nullptr, 0, table.data()) != UTM_EINVAL;
    wrong += utm_class_counts_host(cols.data(), 1, 10, 4, good.data(), 3, nullptr, 2, table.data()) != UTM_EINVAL;
    wrong += utm_class_counts_host(cols.data(), 1, 10, 4, good.data(), 3, twice, 2, table.data()) != UTM_EINVAL;
    wrong += utm_class_counts_host(cols.data(), 1, 10, 4, good.data(), 3, beyond, 2, table.data()) != UTM_EINVAL;
    wrong += utm_class_counts_host(cols.data(), 1, 65, 4, good.data(), 3, nullptr, 0, table.data()) != UTM_EINVAL;
    for (int64_t x : table) wrong += x != -77;
    if (wrong) fprintf(stderr, "%d refusals wrong or the table touched\n", wrong);
    return wrong;
}

int main()
{
    const uint64_t sizes[] = {1, 63, 64, 65, 8191, 8192, 8193, 40000};
    const uint32_t samps[] = {1, 5, 17};
    const int32_t classes[] = {1, 2, 9, 300, UTM_CLASSES_MAX};
    long checked = 0;
    for (uint64_t n_var : sizes)
        for (uint32_t n_samp : samps)
            for (int32_t n_classes : classes) {
                const int family = (int)(checked % 4), list_kind = (int)(checked / 4 % 3);
                if (check(n_var, n_samp, n_classes, family, list_kind)) return 1;
                ++checked;
            }
    for (int i = 0; i < 300; ++i) {  // random shapes
        const uint64_t n_var = 1 + next64() % 3000;
        const uint32_t n_samp = 1 + (uint32_t)(next64() % 20);
        const int32_t n_classes = 1 + (int32_t)(next64() % (i % 10 ? 64 : UTM_CLASSES_MAX));
        if (check(n_var, n_samp, n_classes, i % 4, i % 3)) return 1;
        ++checked;
    }
    if (refusals()) return 1;
    printf("utm_class_counts_host: %ld cases equal the bit loop, the refusals leave the table\n", checked);
    return 0;
}
