// Stand-alone check of utm_coverage_bound_host for a sanitizer build of the HOST code (runs on the CPU, no GPU call):
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -I include \
//         utmos_amd/csrc/utmos_hip.hip tools/bound_host_check.cpp -ldl -o bound_host_check && ./bound_host_check
// The sizes of tests/test_bound_host.py, exact-size buffers (so that any access past them is caught), against a loop over
// dense rows that restates include/utmos_hip.h's definition variant by variant.
#include <algorithm>
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
    const int64_t Q = 65536;
    const uint64_t sizes[] = {1, 63, 64, 65, 8191};
    const uint32_t samples[] = {1, 17, 70};
    const int32_t iters = 12;
    long checked = 0;
    for (uint64_t n_var : sizes)
        for (uint32_t n : samples)
            for (int form = 0; form < 3; ++form) {  // period 2 / step0 1 / a stride wider than the words in use, with `given`
                const uint64_t words = (n_var + 63) / 64, wp = words + (form == 2 ? 3 : 0);
                const uint32_t step0 = form == 1 ? 1 : 0, period = form == 1 ? 0 : 2;
                std::vector<unsigned char> dense((size_t)n_var * n);
                for (uint64_t v = 0; v < n_var; ++v) {
                    for (uint32_t s = 0; s < n; ++s) dense[v * n + s] = next64() % 6 == 0;
                    dense[v * n + next64() % n] = 1;
                }
                std::vector<uint64_t> cols((size_t)n * wp, 0);
                for (uint64_t v = 0; v < n_var; ++v)
                    for (uint32_t s = 0; s < n; ++s)
                        if (dense[v * n + s]) cols[(size_t)s * wp + (v >> 6)] |= 1ull << (v & 63);
                // the candidates: every sample, shuffled, without the last two (when there are that many)
                std::vector<uint32_t> cand(n);
                for (uint32_t s = 0; s < n; ++s) cand[s] = s;
                for (uint32_t s = n; s > 1; --s) std::swap(cand[s - 1], cand[next64() % s]);
                const uint32_t dropped = cand[n - 1];
                if (n > 2) cand.resize(n - 2);
                std::vector<uint32_t> given;
                if (form == 2 && n > 2) given = {cand[0], dropped};  // (cand[0] sits in both lists, `dropped` only in this one)
                const uint64_t n_c = cand.size();
                for (int64_t k : {(int64_t)1, (int64_t)5, (int64_t)n_c, (int64_t)n_c + 3}) {
                    std::vector<int64_t> hist((size_t)iters, 7), want_hist((size_t)iters, 0);
                    std::vector<uint32_t> lambda((size_t)n_var, 7), want_lambda((size_t)n_var, 0);
                    int64_t bound = 7, n_live = 7;
                    int32_t best = 7;
                    const int rc = utm_coverage_bound_host(cols.data(), wp, n_var, n, cand.data(), n_c, given.empty() ? nullptr : given.data(),
                                                           given.size(), k, iters, step0, period, hist.data(), &bound, &best, &n_live,
                                                           lambda.data());
                    if (rc != UTM_OK) {
                        fprintf(stderr, "n_var %llu n %u form %d k %lld: rc %d (%s)\n", (unsigned long long)n_var, n, form, (long long)k, rc,
                                utm_last_error());
                        return 1;
                    }
                    // the definition, variant by variant
                    std::vector<unsigned char> live((size_t)n_var, 1);
                    int64_t want_live = 0;
                    for (uint64_t v = 0; v < n_var; ++v) {
                        for (uint32_t g : given)
                            if (dense[v * n + g]) live[v] = 0;
                        want_live += live[v];
                        want_lambda[v] = live[v] ? (uint32_t)Q : 0u;
                    }
                    const int64_t kk = std::min<int64_t>(k, (int64_t)n_c);
                    const int64_t s0 = step0 ? step0 : Q / 4, per = period ? period : std::max(1, iters / 14);
                    for (int32_t t = 0; t < iters; ++t) {
                        std::vector<int64_t> s((size_t)n_c, 0);
                        for (uint64_t j = 0; j < n_c; ++j)
                            for (uint64_t v = 0; v < n_var; ++v)
                                if (live[v] && dense[v * n + cand[j]]) s[j] += want_lambda[v];
                        std::vector<uint64_t> order((size_t)n_c);
                        for (uint64_t j = 0; j < n_c; ++j) order[j] = j;
                        std::stable_sort(order.begin(), order.end(), [&](uint64_t a, uint64_t b) { return s[a] > s[b]; });
                        int64_t L = 0;
                        for (uint64_t v = 0; v < n_var; ++v)
                            if (live[v]) L += Q - (int64_t)want_lambda[v];
                        for (int64_t r = 0; r < kk; ++r) L += s[order[(size_t)r]];
                        want_hist[(size_t)t] = L;
                        const int64_t shift = std::min<int64_t>(63, t / per), eta = std::max<int64_t>(1, s0 >> shift);
                        for (uint64_t v = 0; v < n_var; ++v) {
                            if (!live[v]) continue;
                            int64_t c = 0;
                            for (int64_t r = 0; r < kk; ++r) c += dense[v * n + cand[order[(size_t)r]]];
                            want_lambda[v] = (uint32_t)std::min<int64_t>(Q, std::max<int64_t>(0, (int64_t)want_lambda[v] - eta * (c - 1)));
                        }
                    }
                    int64_t want_bound = want_hist[0] / Q;
                    int32_t want_best = 0;
                    for (int32_t t = 1; t < iters; ++t)
                        if (want_hist[(size_t)t] / Q < want_bound) want_bound = want_hist[(size_t)t] / Q, want_best = t;
                    want_bound = std::min(want_bound, want_live);
                    if (hist != want_hist || lambda != want_lambda || bound != want_bound || best != want_best || n_live != want_live) {
                        fprintf(stderr, "n_var %llu n %u form %d k %lld: the outputs differ\n", (unsigned long long)n_var, n, form, (long long)k);
                        return 1;
                    }
                    ++checked;
                }
            }
    // refusals leave the outputs alone
    {
        std::vector<uint64_t> cols(4, 0);
        int64_t hist[3] = {7, 7, 7}, bound = 7;
        const uint32_t twice[2] = {1, 1}, far[1] = {4};
        if (utm_coverage_bound_host(cols.data(), 1, 10, 4, twice, 2, nullptr, 0, 2, 3, 0, 0, hist, &bound, nullptr, nullptr, nullptr) != UTM_EINVAL ||
            utm_coverage_bound_host(cols.data(), 1, 10, 4, far, 1, nullptr, 0, 2, 3, 0, 0, hist, &bound, nullptr, nullptr, nullptr) != UTM_EINVAL ||
            utm_coverage_bound_host(cols.data(), 1, 10, 4, nullptr, 0, nullptr, 0, 0, 3, 0, 0, hist, &bound, nullptr, nullptr, nullptr) != UTM_EINVAL ||
            utm_coverage_bound_host(cols.data(), 1, 10, 4, nullptr, 0, nullptr, 0, 2, 0, 0, 0, hist, &bound, nullptr, nullptr, nullptr) != UTM_EINVAL ||
            utm_coverage_bound_host(cols.data(), 1, 10, 4, nullptr, 0, nullptr, 0, 2, 3, 65537, 0, hist, &bound, nullptr, nullptr, nullptr) != UTM_EINVAL ||
            utm_coverage_bound_host(cols.data(), 1, 10, 4, nullptr, 0, nullptr, 0, 2, 3, 0, 0, nullptr, &bound, nullptr, nullptr, nullptr) != UTM_EINVAL ||
            hist[0] != 7 || hist[2] != 7 || bound != 7) {
            fprintf(stderr, "a refusal is missing or wrote an output\n");
            return 1;
        }
    }
    printf("utm_coverage_bound_host: %ld cases equal the loop over dense rows\n", checked);
    return 0;
}
