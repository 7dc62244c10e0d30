// Stand-alone check of utm_filter_columns_host for a sanitizer build of the HOST code (runs on the CPU, no GPU call):
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -I include \
//         utmos_amd/csrc/utmos_hip.hip tools/filter_host_check.cpp -ldl -o filter_host_check && ./filter_host_check
// Every size and mask family of tests/test_filter_host.py, 70 columns, exact-size buffers (so that any access past them is
// caught), against a bit-by-bit loop.
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

int main()
{
    const uint64_t sizes[] = {1, 63, 64, 65, 8191, 8192, 8193, 32767, 32768, 32769, 100003};
    const uint32_t n_cols = 70;
    long checked = 0;
    for (uint64_t n_var : sizes) {
        const uint64_t wp = (n_var + 63) / 64;
        std::vector<uint64_t> cols((size_t)n_cols * wp);
        for (auto &w : cols) w = next64() & next64();
        if (n_var & 63)
            for (uint32_t c = 0; c < n_cols; ++c) cols[(size_t)c * wp + wp - 1] &= (1ull << (n_var & 63)) - 1;
        for (int family = 0; family < 9; ++family) {
            std::vector<uint64_t> keep(wp, 0);
            for (uint64_t v = 0; v < n_var; ++v) {
                bool k = false;
                switch (family) {
                case 0: k = true; break;
                case 1: k = false; break;
                case 2: k = v == 0; break;
                case 3: k = v == n_var - 1; break;
                case 4: k = v & 1; break;
                case 5: k = next64() % 100 < 3; break;
                case 6: k = next64() & 1; break;
                case 7: k = (v >> 6) & 1; break;
                default: k = (v & 63) < (v >> 6) % 65; break;
                }
                if (k) keep[v >> 6] |= 1ull << (v & 63);
            }
            uint64_t kept = 0;
            for (uint64_t v = 0; v < n_var; ++v) kept += keep[v >> 6] >> (v & 63) & 1;
            if (n_var & 63) keep[wp - 1] |= ~0ull << (n_var & 63);  // garbage above n_var: ignored
            const uint64_t wp_out = (kept + 63) / 64;
            std::vector<uint64_t> out((size_t)n_cols * wp_out, 0x5555555555555555ull), want((size_t)n_cols * wp_out, 0);
            uint64_t got_kept = ~0ull;
            const int rc = utm_filter_columns_host(cols.data(), wp, n_var, n_cols, keep.data(), out.data(), wp_out, &got_kept);
            if (rc != UTM_OK || got_kept != kept) {
                fprintf(stderr, "n_var %llu family %d: rc %d kept %llu want %llu\n", (unsigned long long)n_var, family, rc,
                        (unsigned long long)got_kept, (unsigned long long)kept);
                return 1;
            }
            for (uint32_t c = 0; c < n_cols; ++c) {
                uint64_t at = 0;
                for (uint64_t v = 0; v < n_var; ++v)
                    if (keep[v >> 6] >> (v & 63) & 1) {
                        want[(size_t)c * wp_out + (at >> 6)] |= (cols[(size_t)c * wp + (v >> 6)] >> (v & 63) & 1) << (at & 63);
                        ++at;
                    }
            }
            if (out != want) {
                fprintf(stderr, "n_var %llu family %d: columns differ\n", (unsigned long long)n_var, family);
                return 1;
            }
            ++checked;
        }
    }
    printf("utm_filter_columns_host: %ld cases equal the bit loop\n", checked);
    return 0;
}
