// BCF batches on the VCF parse context (utm_vcf_parse_bcf): host side of bcf.hip.h.  Restates the genotype half of the
// reference's convert (utmos/convert.py:43-88) for the records of a BCF2 stream whose header the caller has read.
//
// A batch is the carry of the previous one, the caller's prefix, then new stream bytes -- whole BGZF members inflated on
// the device (as in utm_vcf_parse_bgzf) or bytes the caller has inflated.  BCF has no newline: k_bcf_chain follows the
// length prefixes on the device and says where the last whole record ends; the bytes behind it are copied on the device
// to the head of the other slot's text, the way the BGZF path carries an unfinished line.
#pragma once

extern "C" int utm_vcf_parse_bcf(utm_vcf *p, const uint8_t *prefix, uint64_t prefix_bytes, const uint8_t *packed,
                                 uint64_t packed_bytes, const uint32_t *members, uint64_t n_members, uint32_t gt_key,
                                 uint32_t flags, uint64_t *n_records, uint64_t *carry_bytes)
{
    BATCH_CTX(p, "vcf");
    if (!n_records || !carry_bytes) return fail(UTM_EINVAL, "n_records or carry_bytes is NULL");
    if ((prefix_bytes && !prefix) || (packed_bytes && !packed) || (n_members && !members))
        return fail(UTM_EINVAL, "prefix, packed or members is NULL");
    if (flags & ~(UTM_BGZF_FIRST | UTM_BGZF_LAST)) return fail(UTM_EINVAL, "unknown flags 0x%x", flags);
    VcfSlot *s;
    TRY(p->free_slot("utm_vcf_fetch", &s));
    if (flags & UTM_BGZF_FIRST) p->carry = 0;
    const bool last = flags & UTM_BGZF_LAST;
    const u64 carry = p->carry;
    p->carry = 0;  // (set again once this batch has succeeded)
    if (packed_bytes > UTM_VCF_MAX_BATCH) return fail(UTM_EINVAL, "a batch of %llu bytes (at most 2^32 - 64)", (unsigned long long)packed_bytes);
    u64 n = carry + prefix_bytes;  // the text: carry, prefix, then the members' text or the caller's bytes
    if (n_members) {
        TRY(s->d_packed.reserve(packed_bytes, s->h_text.cap));
        TRY(s->d_members.reserve(n_members, 1024));
        TRY(s->d_mstat.reserve(n_members, 1024));
        TRY(s->h_members.reserve(n_members, 1024));
        TRY(vcf_member_table(s, members, n_members, packed_bytes, &n));
    } else {
        n += packed_bytes;
        if (n + 1 > UTM_VCF_MAX_BATCH) return fail(UTM_EINVAL, "a batch of more than 2^32 - 64 stream bytes");
    }
    if (packed && packed != s->h_text && packed_bytes) {
        TRY(s->h_text.grow(packed_bytes));
        memcpy(s->h_text, packed, packed_bytes);
    }
    TRY(vcf_slot_ready(p, s));
    TRY(s->d_text.grow(n + VCF_TEXT_PAD, carry, s->stream));
    TRY(s->d_nl.reserve(n / 32 + 1, 1024));  // record offsets: a record is 32 bytes at least
    s->bgzf = true;                          // (the timing split of a batch with an inflate phase)
    HIP_TRY(hipEventRecord(s->ev[0], s->stream));
    if (n_members) {
        HIP_TRY(hipMemcpyAsync(s->d_packed, s->h_text, packed_bytes, hipMemcpyHostToDevice, s->stream));
        HIP_TRY(hipMemcpyAsync(s->d_members, s->h_members, n_members * sizeof(InfMember), hipMemcpyHostToDevice, s->stream));
    } else if (packed_bytes) {
        HIP_TRY(hipMemcpyAsync(s->d_text + carry + prefix_bytes, s->h_text, packed_bytes, hipMemcpyHostToDevice, s->stream));
    }
    if (prefix_bytes) HIP_TRY(hipMemcpyAsync(s->d_text + carry, prefix, prefix_bytes, hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipEventRecord(s->ev_h2d, s->stream));
    // misc: [0] records, [1] first failing record, [2] end of the last whole record, [3] first failing member
    HIP_TRY(hipMemsetAsync(s->d_misc, 0, 4 * sizeof(unsigned), s->stream));
    HIP_TRY(hipMemsetAsync(s->d_misc + 1, 0xFF, sizeof(unsigned), s->stream));
    HIP_TRY(hipMemsetAsync(s->d_misc + 3, 0xFF, sizeof(unsigned), s->stream));
    if (n_members) k_bgzf_inflate<<<(unsigned)n_members, INF_THREADS, 0, s->stream>>>(s->d_packed, s->d_members, s->d_text, s->d_mstat, s->d_misc);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(s->ev[1], s->stream));
    if (n) {
        k_bcf_chain<<<1, VCF_THREADS, 0, s->stream>>>(s->d_text, (unsigned)n, s->d_nl, s->d_misc);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(s->ev[2], s->stream));
    HIP_TRY(hipMemcpyAsync(s->h_misc, s->d_misc, 4 * sizeof(unsigned), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));  // records, carry, the first failing member
    if (s->h_misc[3] != 0xFFFFFFFFu) return vcf_member_failure(s, s->h_misc[3]);
    // a prefix the chain could not follow: nothing behind it in the batch is known, so the file ends here
    if (n && s->h_misc[1] != 0xFFFFFFFFu) return fail(UTM_EINVAL, "record %u of the batch: %s", s->h_misc[1], vcf_error_text(BCF_E_SHARED));
    const u64 n_rec = n ? s->h_misc[0] : 0, cut = n ? s->h_misc[2] : 0;
    const u64 carry_next = n - cut;
    if (last && carry_next) return fail(UTM_EINVAL, "truncated record: the stream ends %llu bytes into record %llu of the batch", (unsigned long long)carry_next, (unsigned long long)n_rec);
    if (carry_next) {  // the unfinished record: to the head of the other slot's text, on that slot's stream
        VcfSlot *o = p->other(s);
        TRY(o->d_text.grow(carry_next + VCF_TEXT_PAD, 0, o->stream));
        HIP_TRY(hipEventRecord(s->ev[3], s->stream));
        HIP_TRY(hipStreamWaitEvent(o->stream, s->ev[3], 0));
        HIP_TRY(hipMemcpyAsync(o->d_text, s->d_text + cut, carry_next, hipMemcpyDeviceToDevice, o->stream));
        HIP_TRY(hipEventRecord(o->ev_carry, o->stream));
        s->carry_out = true;
    }
    TRY(bcf_parse_records(p, s, n, n_rec, gt_key));
    p->carry = carry_next;
    *n_records = n_rec;
    *carry_bytes = carry_next;
    return UTM_OK;
}

// k_bcf_chain's walk and k_bcf_parse's decode built for the CPU, one record after the other: stream[0, n_bytes) = the
// bytes after the header.  Tests and tools check it against utmos_amd/bcfio.py without a GPU.
extern "C" int utm_bcf_parse_host(const uint8_t *stream, uint64_t n_bytes, uint32_t n_samples, uint32_t gt_key,
                                  uint64_t max_records, uint8_t *rows, double *af, uint32_t *n_het, uint32_t *n_hom,
                                  uint8_t *flags, uint64_t *n_records, uint64_t *carry_bytes)
{
    if (!n_records || !carry_bytes || (n_bytes && !stream)) return fail(UTM_EINVAL, "stream, n_records or carry_bytes is NULL");
    if (n_samples == 0 || n_samples > UTM_VCF_MAX_SAMPLES) return fail(UTM_EINVAL, "n_samples %u not in [1, %u]", n_samples, (unsigned)UTM_VCF_MAX_SAMPLES);
    if (n_bytes > UTM_VCF_MAX_BATCH) return fail(UTM_EINVAL, "a stream of %llu bytes (at most 2^32 - 64)", (unsigned long long)n_bytes);
    // the chain
    std::vector<u64> offs;
    u64 q = 0;
    while (q + 8 <= n_bytes) {
        u64 next = 0;
        const int hop = bcf_hop(bcf_rd(stream + q, 4), bcf_rd(stream + q + 4, 4), q, n_bytes, &next);
        if (hop == BCF_HOP_CARRY) break;
        offs.push_back(q);
        q = hop == BCF_HOP_BAD ? n_bytes : next;
    }
    *n_records = offs.size();
    *carry_bytes = n_bytes - q;
    if (!rows && !af && !n_het && !n_hom && !flags) return UTM_OK;  // the counts only
    if (!rows || !af || !n_het || !n_hom || !flags) return fail(UTM_EINVAL, "output is NULL");
    if (offs.size() > max_records) return fail(UTM_EINVAL, "%llu records, room for %llu", (unsigned long long)offs.size(), (unsigned long long)max_records);
    // the records
    const u64 row_bytes = (n_samples + 7) / 8;
    std::vector<unsigned> cnt(VCF_MAX_ALT + 1);
    for (u64 r = 0; r < offs.size(); ++r) {
        BcfGt g = {0, 0, 0, 1};
        const int err = bcf_find_gt(stream, offs[r], n_bytes, n_samples, gt_key, &g);
        if (err) return fail(UTM_EINVAL, "record %llu of the batch: %s", (unsigned long long)r, vcf_error_text((unsigned)err));
        std::fill(cnt.begin(), cnt.begin() + g.n_alt + 1, 0u);
        uint8_t *row = rows + r * row_bytes;
        memset(row, 0, row_bytes);
        unsigned het = 0, hom = 0;
        if (g.width)
            for (u64 j = 0; j < n_samples; ++j) {
                const int c = bcf_cell(stream + g.at + j * g.len * g.width, g, cnt.data());
                het += c == 1;
                hom += c == 2;
                if (c) row[j >> 3] |= (uint8_t)(0x80u >> (j & 7));
            }
        unsigned total = 0, mx = 0;
        for (unsigned a = 0; a <= g.n_alt; ++a) {
            total += cnt[a];
            if (a) mx = std::max(mx, cnt[a]);
        }
        af[r] = total ? (double)mx / (double)total : 0.0;
        n_het[r] = het;
        n_hom[r] = hom;
        flags[r] = (cnt[1] == 1 || cnt[0] == 1) ? UTM_VCF_SINGLETON : 0;
    }
    return UTM_OK;
}
