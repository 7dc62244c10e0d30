// Stand-alone check of utm_multi_select_host and utm_multi_keep_host for a sanitizer build of the HOST code (runs on the
// CPU, no GPU call):
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -I include \
//         utmos_amd/csrc/utmos_hip.hip tools/multi_host_check.cpp -ldl -o multi_host_check && ./multi_host_check
// The sizes of tests/test_multi_host.py, exact-size buffers (so that any access past them is caught), against a bit-by-bit
// greedy loop over dense rows.
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

static uint64_t mix(uint64_t z)
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

int main()
{
    const uint64_t sizes[] = {1, 63, 64, 65, 1000};
    const uint32_t samples[] = {1, 17, 70};
    const uint32_t reps[] = {1, 2, 63, 64, 65};
    long checked = 0;
    for (uint64_t n_var : sizes)
        for (uint32_t n : samples)
            for (uint32_t n_rep : reps) {
                const uint64_t wp = (n_var + 63) / 64;
                // dense[v * n + s]; every variant has a carrier
                std::vector<unsigned char> dense((size_t)n_var * n);
                for (uint64_t v = 0; v < n_var; ++v) {
                    for (uint32_t s = 0; s < n; ++s) dense[v * n + s] = next64() % 8 == 0;
                    dense[v * n + next64() % n] = 1;
                }
                std::vector<uint64_t> cols((size_t)n * wp, 0);
                for (uint64_t v = 0; v < n_var; ++v)
                    for (uint32_t s = 0; s < n; ++s)
                        if (dense[v * n + s]) cols[(size_t)s * wp + (v >> 6)] |= 1ull << (v & 63);
                std::vector<uint8_t> state((size_t)n_rep * n);
                for (auto &x : state) {
                    const uint64_t r = next64() % 6;
                    x = r < 4 ? 1 : r == 4 ? 0 : 2;
                }
                // masks: all ones, all zero, the hashed half, one variant -- in turn; garbage above n_var
                std::vector<uint64_t> keep((size_t)n_rep * wp, 0);
                const uint64_t seed = next64(), first = next64() >> 8;
                for (uint32_t b = 0; b < n_rep; ++b) {
                    uint64_t *kw = keep.data() + (size_t)b * wp;
                    switch (b % 4) {
                    case 0: for (uint64_t w = 0; w < wp; ++w) kw[w] = ~0ull; break;
                    case 1: break;
                    case 2:
                        if (utm_multi_keep_host(seed, b, first, n_var, 1ull << 31, kw) != UTM_OK) return 1;
                        for (uint64_t v = 0; v < n_var; ++v) {
                            const uint64_t z = mix(seed + 0x9E3779B97F4A7C15ull * (first + v + 1) + 0xD1B54A32D192ED03ull * ((uint64_t)b + 1));
                            if ((kw[v >> 6] >> (v & 63) & 1) != ((z >> 32) < (1ull << 31))) {
                                fprintf(stderr, "hashed mask: variant %llu of replicate %u differs\n", (unsigned long long)v, b);
                                return 1;
                            }
                        }
                        if ((n_var & 63) && kw[wp - 1] >> (n_var & 63)) {
                            fprintf(stderr, "hashed mask: bits above n_var\n");
                            return 1;
                        }
                        break;
                    default: {
                        const uint64_t v = next64() % n_var;
                        kw[v >> 6] = 1ull << (v & 63);
                        break;
                    }
                    }
                    if (n_var & 63) kw[wp - 1] |= ~0ull << (n_var & 63);
                }
                const int64_t k = (int64_t)n + 2;
                std::vector<int32_t> order((size_t)n_rep * k, 7), want_order((size_t)n_rep * k, -1);
                std::vector<int64_t> gain((size_t)n_rep * k, 7), want_gain((size_t)n_rep * k, 0), kept(n_rep, 7), want_kept(n_rep, 0), done(n_rep, 7),
                    want_done(n_rep, 0);
                const int rc = utm_multi_select_host(cols.data(), wp, n_var, n, n_rep, state.data(), keep.data(), k, order.data(), gain.data(),
                                                     kept.data(), done.data());
                if (rc != UTM_OK) {
                    fprintf(stderr, "n_var %llu n %u reps %u: rc %d (%s)\n", (unsigned long long)n_var, n, n_rep, rc, utm_last_error());
                    return 1;
                }
                for (uint32_t b = 0; b < n_rep; ++b) {
                    std::vector<unsigned char> live(n_var);
                    std::vector<uint8_t> st(state.begin() + (size_t)b * n, state.begin() + (size_t)(b + 1) * n);
                    for (uint64_t v = 0; v < n_var; ++v) {
                        live[v] = keep[(size_t)b * wp + (v >> 6)] >> (v & 63) & 1;
                        want_kept[b] += live[v];
                        for (uint32_t s = 0; s < n; ++s)
                            if (st[s] == 0 && dense[v * n + s]) live[v] = 0;
                    }
                    int64_t tot = 0;
                    for (int64_t row = 0; row < k; ++row) {
                        int64_t best = 0, best_s = -1;
                        for (uint32_t s = 0; s < n; ++s) {
                            if (st[s] != 1) continue;
                            int64_t cnt = 0;
                            for (uint64_t v = 0; v < n_var; ++v) cnt += live[v] & dense[v * n + s];
                            if (cnt > best) best = cnt, best_s = s;
                        }
                        if (best_s < 0) break;
                        want_order[(size_t)b * k + row] = (int32_t)best_s;
                        want_gain[(size_t)b * k + row] = best;
                        want_done[b] = row + 1;
                        tot += best;
                        st[best_s] = 0;
                        for (uint64_t v = 0; v < n_var; ++v)
                            if (dense[v * n + best_s]) live[v] = 0;
                        if (tot >= want_kept[b]) break;
                    }
                }
                if (order != want_order || gain != want_gain || kept != want_kept || done != want_done) {
                    fprintf(stderr, "n_var %llu n %u reps %u: rows differ\n", (unsigned long long)n_var, n, n_rep);
                    return 1;
                }
                ++checked;
            }
    printf("utm_multi_select_host / utm_multi_keep_host: %ld cases equal the bit loop\n", checked);
    return 0;
}
