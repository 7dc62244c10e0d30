// Stand-alone check of utm_bcf_parse_host for a sanitizer build of the HOST code (runs on the CPU, no GPU call):
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -I include \
//         utmos_amd/csrc/utmos_hip.hip tools/bcf_host_check.cpp -ldl -o bcf_host_check && ./bcf_host_check
// Seeded BCF record streams (every GT width, per-sample lengths 0..5 and 17, sentinels, a field in front of GT with the
// length-15 overflow) in exact-size buffers, so that any access past them is caught: good streams against a cell-by-cell
// loop written here, then the same streams truncated at every length of a window and with bytes overwritten, where the
// call must return UTM_OK or UTM_EINVAL and nothing else may happen.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

static void put32(std::vector<uint8_t> &b, uint32_t v)
{
    for (int i = 0; i < 4; ++i) b.push_back((uint8_t)(v >> (8 * i)));
}
static void put_value(std::vector<uint8_t> &b, uint32_t v, unsigned width)
{
    for (unsigned i = 0; i < width; ++i) b.push_back((uint8_t)(v >> (8 * i)));
}

struct Want {
    std::vector<uint8_t> row;
    double af;
    uint32_t het, hom;
    uint8_t flag;
};

static const uint32_t GT_KEY = 9;

// One record of n_samp samples appended to `out`; what the reader must make of it in `want`.
static void make_record(std::vector<uint8_t> &out, uint32_t n_samp, Want *want)
{
    const unsigned width = 1u << (next64() % 3);  // 1, 2, 4
    const unsigned lens[] = {0, 1, 2, 2, 2, 3, 5, 17};
    const unsigned len = lens[next64() % 8];
    const uint32_t n_allele = 1 + (uint32_t)(next64() % (width == 1 ? 40 : 300));
    const uint32_t n_alt = n_allele > 2 ? n_allele - 1 : 1;
    const uint32_t miss_s = 1u << (8 * width - 1), eov = miss_s + 1;
    std::vector<uint8_t> shared, indiv;
    put32(shared, 0), put32(shared, 5), put32(shared, 1), put32(shared, 0x7F800001u);
    put32(shared, n_allele << 16);
    put32(shared, 2u << 24 | n_samp);
    for (unsigned i = next64() % 40; i; --i) shared.push_back((uint8_t)next64());  // ID, alleles, FILTER, INFO: skipped by l_shared
    // a field in front of GT: key 3, int16 x 20 (length-15 overflow)
    indiv.push_back(0x11), indiv.push_back(3);
    indiv.push_back(0xF2), indiv.push_back(0x11), indiv.push_back(20);
    for (uint64_t i = 0; i < (uint64_t)n_samp * 20 * 2; ++i) indiv.push_back((uint8_t)next64());
    // GT
    indiv.push_back(0x11), indiv.push_back((uint8_t)GT_KEY);
    if (len < 15) indiv.push_back((uint8_t)(len << 4 | (width == 1 ? 1 : width == 2 ? 2 : 3)));
    else indiv.push_back((uint8_t)(0xF0 | (width == 1 ? 1 : width == 2 ? 2 : 3))), indiv.push_back(0x11), indiv.push_back((uint8_t)len);
    std::vector<uint64_t> cnt(n_alt + 1, 0);
    want->row.assign((n_samp + 7) / 8, 0);
    want->het = want->hom = 0;
    for (uint32_t j = 0; j < n_samp; ++j) {
        unsigned ploidy = 0;
        bool ended = false, missing = false, diff = false;
        uint32_t first = 0;
        for (unsigned k = 0; k < len; ++k) {
            uint32_t v;
            const unsigned pick = next64() % 16;
            if (pick == 0) v = eov;
            else if (pick == 1) v = miss_s;
            else if (pick == 2) v = (uint32_t)(next64() & 1);  // allele 0 of the encoding: missing
            else v = (uint32_t)(((next64() % (n_alt + 2)) + 1) << 1 | (next64() & 1));  // alleles 0 .. n_alt + 1
            if (width < 4 && v >= miss_s && v != miss_s && v != eov) v = 2;
            put_value(indiv, v, width);
            if (ended) continue;
            if (v == eov) {
                ended = true;
                continue;
            }
            const bool miss = v == miss_s || (v >> 1) == 0;
            const uint32_t a = (v >> 1) - 1;
            if (!miss && a <= n_alt) ++cnt[a];
            if (ploidy == 0) first = a;
            else if (a != first) diff = true;
            missing |= miss;
            ++ploidy;
        }
        const bool called = ploidy >= 2 && !missing;
        const bool het = called && diff, hom = called && !diff && first > 0;
        want->het += het;
        want->hom += hom;
        if (het || hom) want->row[j >> 3] |= (uint8_t)(0x80 >> (j & 7));
    }
    uint64_t total = 0, mx = 0;
    for (uint32_t a = 0; a <= n_alt; ++a) {
        total += cnt[a];
        if (a && cnt[a] > mx) mx = cnt[a];
    }
    want->af = total ? (double)mx / (double)total : 0.0;
    want->flag = (cnt[1] == 1 || cnt[0] == 1) ? UTM_VCF_SINGLETON : 0;
    put32(out, (uint32_t)shared.size()), put32(out, (uint32_t)indiv.size());
    out.insert(out.end(), shared.begin(), shared.end());
    out.insert(out.end(), indiv.begin(), indiv.end());
}

// The call on an exact-size copy of data[0, n).  Returns its code; the outputs hold room for max_rec records.
static int run(const uint8_t *data, size_t n, uint32_t n_samp, size_t max_rec, std::vector<uint8_t> &rows, std::vector<double> &af,
               std::vector<uint32_t> &het, std::vector<uint32_t> &hom, std::vector<uint8_t> &flags, uint64_t *n_rec, uint64_t *carry)
{
    uint8_t *exact = (uint8_t *)malloc(n ? n : 1);
    memcpy(exact, data, n);
    rows.assign(max_rec * ((n_samp + 7) / 8) + 1, 0xAA);
    af.assign(max_rec + 1, -1.0);
    het.assign(max_rec + 1, 0), hom.assign(max_rec + 1, 0), flags.assign(max_rec + 1, 0);
    const int rc = utm_bcf_parse_host(exact, n, n_samp, GT_KEY, max_rec, rows.data(), af.data(), het.data(), hom.data(), flags.data(), n_rec, carry);
    free(exact);
    return rc;
}

int main()
{
    const uint32_t sizes[] = {1, 7, 8, 9, 63, 65, 300};
    long good = 0, damaged = 0, refused = 0;
    for (uint32_t n_samp : sizes) {
        for (int round = 0; round < 6; ++round) {
            const size_t n_rec = 1 + next64() % 12;
            std::vector<uint8_t> stream;
            std::vector<Want> want(n_rec);
            std::vector<size_t> ends;
            for (size_t r = 0; r < n_rec; ++r) {
                make_record(stream, n_samp, &want[r]);
                ends.push_back(stream.size());
            }
            std::vector<uint8_t> rows, flags;
            std::vector<double> af;
            std::vector<uint32_t> het, hom;
            uint64_t got_rec = 0, carry = 0;
            int rc = run(stream.data(), stream.size(), n_samp, n_rec, rows, af, het, hom, flags, &got_rec, &carry);
            if (rc != UTM_OK || got_rec != n_rec || carry != 0) {
                fprintf(stderr, "n_samp %u round %d: rc %d (%s) records %llu of %zu carry %llu\n", n_samp, round, rc, utm_last_error(),
                        (unsigned long long)got_rec, n_rec, (unsigned long long)carry);
                return 1;
            }
            const size_t rb = (n_samp + 7) / 8;
            for (size_t r = 0; r < n_rec; ++r) {
                if (memcmp(rows.data() + r * rb, want[r].row.data(), rb) || af[r] != want[r].af || het[r] != want[r].het ||
                    hom[r] != want[r].hom || flags[r] != want[r].flag) {
                    fprintf(stderr, "n_samp %u round %d record %zu differs: af %.17g want %.17g het %u/%u hom %u/%u flag %u/%u\n", n_samp, round, r,
                            af[r], want[r].af, het[r], want[r].het, hom[r], want[r].hom, flags[r], want[r].flag);
                    return 1;
                }
            }
            ++good;
            // truncated at every length of a window around a record border and at random lengths: whole records + carry
            for (int k = 0; k < 80; ++k) {
                const size_t border = ends[next64() % n_rec];
                size_t cut = k < 40 ? border - (border < 20 ? border : 20) + (size_t)k : next64() % (stream.size() + 1);
                if (cut > stream.size()) cut = stream.size();
                rc = run(stream.data(), cut, n_samp, n_rec, rows, af, het, hom, flags, &got_rec, &carry);
                size_t whole = 0;
                while (whole < n_rec && ends[whole] <= cut) ++whole;
                if (rc != UTM_OK || got_rec != whole || carry != cut - (whole ? ends[whole - 1] : 0)) {
                    fprintf(stderr, "n_samp %u round %d cut %zu: rc %d records %llu want %zu carry %llu\n", n_samp, round, cut, rc,
                            (unsigned long long)got_rec, whole, (unsigned long long)carry);
                    return 1;
                }
                ++damaged;
            }
            // bytes overwritten in the prefixes, the counts and the field headers (and anywhere): any answer but a crash
            for (int k = 0; k < 200; ++k) {
                std::vector<uint8_t> bad = stream;
                const size_t rec0 = (next64() % n_rec) ? ends[next64() % n_rec] % stream.size() : 0;
                const int hits = 1 + (int)(next64() % 3);
                for (int h = 0; h < hits; ++h) {
                    const size_t at = (next64() & 1) ? (rec0 + next64() % 40) % bad.size() : next64() % bad.size();
                    bad[at] = (next64() & 3) ? (uint8_t)next64() : (uint8_t)((next64() & 1) ? 0xFF : 0x00);
                }
                // (a damaged prefix may claim more records than there were: the chain's count first, then room for them)
                rc = utm_bcf_parse_host(bad.data(), bad.size(), n_samp, GT_KEY, 0, nullptr, nullptr, nullptr, nullptr, nullptr, &got_rec, &carry);
                if (rc != UTM_OK) return fprintf(stderr, "count call failed: %s\n", utm_last_error()), 1;
                rc = run(bad.data(), bad.size(), n_samp, (size_t)got_rec, rows, af, het, hom, flags, &got_rec, &carry);
                if (rc != UTM_OK && rc != UTM_EINVAL) {
                    fprintf(stderr, "n_samp %u round %d damage %d: rc %d (%s)\n", n_samp, round, k, rc, utm_last_error());
                    return 1;
                }
                refused += rc == UTM_EINVAL;
                ++damaged;
            }
        }
    }
    printf("utm_bcf_parse_host: %ld good streams equal the cell loop, %ld damaged ones answered (%ld refused)\n", good, damaged, refused);
    return 0;
}
