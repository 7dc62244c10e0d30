// VCF parse context (utm_vcf_*): host side of vcf.hip.h and inflate.hip.h.  Restates the genotype half of the
// reference's convert (utmos/convert.py:43-88) for text the caller has already split off its header: inflated on the
// host (utm_vcf_parse) or BGZF members inflated on the device (utm_vcf_parse_bgzf).
//
// Two slots (host_batch.hip.h), each with its own pinned staging, device text and per-record buffers: utm_vcf_parse
// returns once its batch has reached the device and the parse is queued, so the caller fills the other slot's staging
// (inflate, read) while the GPU parses; utm_vcf_fetch then collects the oldest batch.
//
// BGZF batches end at member borders, so a record may run from one batch into the next.  The bytes after the last
// newline of a batch (the carry) are copied on the device to the head of the other slot's text, and the next batch
// inflates after them: the host never sees the text.
#pragma once

struct VcfSlot : BatchSlot<6> {  // events around: H2D (0-1), count + scan (1-2), [host reads the count], write + parse (3-4), D2H (4-5)
    Pinned<unsigned char> h_text;   // staging: the text, or a BGZF batch's compressed bytes
    Scratch<unsigned char> d_text;  // + 64 bytes: 16-byte loads may run past the last record
    Scratch<unsigned> d_blk;
    Scratch<unsigned> d_misc;  // [0] records, [1] first failing record
    Pinned<unsigned> h_misc;
    // per record
    Scratch<unsigned char> d_rows;
    Scratch<unsigned> d_nl, d_het, d_hom, d_status;
    Scratch<double> d_af;
    Pinned<unsigned char> h_rows;
    Pinned<double> h_af;
    Pinned<unsigned> h_het, h_hom, h_status;
    u64 n_rec = 0;
    // BGZF batches: compressed bytes and the member table on the device, a status word per member
    Scratch<unsigned char> d_packed;
    Scratch<InfMember> d_members;
    Pinned<InfMember> h_members;
    Scratch<unsigned> d_mstat;
    hipEvent_t ev_h2d = nullptr;    // BGZF: end of the copies in (ev[0] .. ev_h2d), inflate (ev_h2d .. ev[1])
    hipEvent_t ev_carry = nullptr;  // on this slot's stream: the carry copy into its text is done
    bool bgzf = false;              // the pending batch came through utm_vcf_parse_bgzf
    bool carry_out = false;         // this slot's text is the source of a carry copy on the other stream
    ~VcfSlot()
    {
        if (ev_h2d) (void)hipEventDestroy(ev_h2d);
        if (ev_carry) (void)hipEventDestroy(ev_carry);
    }
};

struct utm_vcf : SlotPair<VcfSlot> {
    int device = 0;
    uint32_t n_samples = 0;
    uint32_t row_words = 0;  // LDS row in the kernel: ceil(S / 32) words
    uint32_t row_bytes = 0;  // packed row: ceil(S / 8) bytes
    double ms[3] = {0, 0, 0};  // H2D, kernels, D2H
    double inflate_ms = 0;     // BGZF inflate kernels
    double find_ms = 0;        // the two parts of ms[1]: finding the records (newline count + scan, or the BCF chain) ...
    double parse_ms = 0;       // ... and parsing them (newline offsets + k_vcf_parse, or k_bcf_parse)
    u64 carry = 0;             // bytes at the head of slot[next]'s text that the next BGZF batch continues
    ~utm_vcf() { idle(device); }
};

static const char *vcf_error_text(unsigned code)
{
    switch (code) {
    case VCF_E_COLUMNS: return "a record with fewer than ten columns";
    case VCF_E_CELLS: return "a record whose sample column count differs from the header's";
    case VCF_E_NO_GT: return "no GT in FORMAT, or a sample cell without its GT subfield";
    case VCF_E_ALLELE: return "a malformed allele token (neither '.' nor an unsigned decimal)";
    case VCF_E_NALT: return "more alt alleles than the parser holds (4096)";
    case VCF_E_HEADER: return "a #CHROM line after the first record";
    case VCF_E_RANGE: return "an allele number above 10^18";
    case BCF_E_SHARED: return "l_shared below 24";
    case BCF_E_TRUNC: return "the record runs past the end of its batch";
    case BCF_E_NSAMPLE: return "a record whose n_sample differs from the header's sample count";
    case BCF_E_NALT: return "more alt alleles than the parser holds (4096)";
    case BCF_E_FIELD: return "a FORMAT field that runs past l_indiv";
    case BCF_E_TYPE: return "an unknown type code";
    case BCF_E_GT_TYPE: return "a GT field that is not of an integer type";
    case BCF_E_NO_GT: return "no GT among the FORMAT fields";
    default: return "unknown record error";
    }
}

static const char *inf_error_text(unsigned code)
{
    switch (code) {
    case INF_E_HEADER: return "not a gzip deflate member header";
    case INF_E_BTYPE: return "invalid block type";
    case INF_E_STORED: return "invalid stored block lengths";
    case INF_E_OVERSUB: return "over-subscribed code lengths";
    case INF_E_INCOMPLETE: return "incomplete code lengths";
    case INF_E_CODE: return "invalid code";
    case INF_E_LENS: return "invalid dynamic block header";
    case INF_E_DIST: return "invalid distance too far back";
    case INF_E_INPUT: return "deflate data runs past the member";
    case INF_E_TRAILING: return "deflate data ends before the member's trailer";
    case INF_E_CRC: return "incorrect data check";
    case INF_E_ISIZE: return "ISIZE above 65536";
    default: return "unknown member error";
    }
}

#define VCF_TEXT_PAD 64  // device text past the end: 16-byte loads may run past the last record

// The slot's text may be written once a carry copy out of it (queued on the other slot's stream) is done.
static int vcf_slot_ready(utm_vcf *p, VcfSlot *s)
{
    if (s->carry_out) {
        HIP_TRY(hipStreamWaitEvent(s->stream, p->other(s)->ev_carry, 0));
        s->carry_out = false;
    }
    return UTM_OK;
}

extern "C" int utm_vcf_create(int device, uint32_t n_samples, uint64_t batch_bytes, utm_vcf **out)
{
    if (!out) return fail(UTM_EINVAL, "out is NULL");
    *out = nullptr;
    if (n_samples == 0 || n_samples > UTM_VCF_MAX_SAMPLES)
        return fail(UTM_EINVAL, "n_samples %u not in [1, %u]", n_samples, (unsigned)UTM_VCF_MAX_SAMPLES);
    if (batch_bytes == 0 || batch_bytes > UTM_VCF_MAX_BATCH) return fail(UTM_EINVAL, "batch_bytes %llu not in [1, 2^32 - 64)", (unsigned long long)batch_bytes);
    TRY(open_device(device));
    if (n_samples > 32768u * 8u)  // rows above 32 KiB of LDS ask for it explicitly
        HIP_TRY(hipFuncSetAttribute((const void *)k_vcf_parse, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)(((n_samples + 31) / 32) * sizeof(unsigned))));
    if (n_samples > 32768u * 8u)
        HIP_TRY(hipFuncSetAttribute((const void *)k_bcf_parse, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)(((n_samples + 31) / 32) * sizeof(unsigned))));
    std::unique_ptr<utm_vcf> p(new utm_vcf());
    p->device = device;
    p->n_samples = n_samples;
    p->row_words = (n_samples + 31) / 32;
    p->row_bytes = (n_samples + 7) / 8;
    for (VcfSlot &s : p->slot) {
        TRY(s.open());
        HIP_TRY(hipEventCreate(&s.ev_h2d));
        HIP_TRY(hipEventCreateWithFlags(&s.ev_carry, hipEventDisableTiming));
        TRY(s.d_misc.reserve(4));
        TRY(s.h_misc.reserve(4));
        TRY(s.h_text.grow(batch_bytes));
        TRY(s.d_text.reserve(batch_bytes + VCF_TEXT_PAD));
        TRY(s.d_blk.reserve((batch_bytes + VCF_BLOCK_BYTES - 1) / VCF_BLOCK_BYTES));
    }
    *out = p.release();
    return UTM_OK;
}

extern "C" int utm_vcf_destroy(utm_vcf *p)
{
    delete p;
    return UTM_OK;
}

extern "C" int utm_vcf_staging(utm_vcf *p, uint64_t n_bytes, uint8_t **buf, uint64_t *cap)
{
    BATCH_CTX(p, "vcf");
    if (!buf || !cap) return fail(UTM_EINVAL, "output is NULL");
    if (n_bytes > UTM_VCF_MAX_BATCH) return fail(UTM_EINVAL, "a batch of %llu bytes (at most 2^32 - 64)", (unsigned long long)n_bytes);
    VcfSlot *s = p->next_slot();
    TRY(s->h_text.grow(n_bytes));  // keeps what it held: a record longer than a batch grows the staging mid-fill
    *buf = s->h_text;
    *cap = s->h_text.cap;
    return UTM_OK;
}

// Room for the results of n_rec records on the device and in pinned memory.
static int vcf_reserve_results(utm_vcf *p, VcfSlot *s, u64 n_rec)
{
    const u64 floor = 1024;
    TRY(s->d_rows.reserve(n_rec * p->row_bytes, floor * p->row_bytes));
    TRY(s->d_het.reserve(n_rec, floor));
    TRY(s->d_hom.reserve(n_rec, floor));
    TRY(s->d_status.reserve(n_rec, floor));
    TRY(s->d_af.reserve(n_rec, floor));
    TRY(s->h_rows.reserve(n_rec * p->row_bytes, floor * p->row_bytes));
    TRY(s->h_af.reserve(n_rec, floor));
    TRY(s->h_het.reserve(n_rec, floor));
    TRY(s->h_hom.reserve(n_rec, floor));
    TRY(s->h_status.reserve(n_rec, floor));
    return UTM_OK;
}

// The parse kernels are queued (between ev[3] and ev[4]): the results are copied back and the batch is queued.
static int vcf_results_back(utm_vcf *p, VcfSlot *s, u64 n_rec)
{
    HIP_TRY(hipEventRecord(s->ev[4], s->stream));
    if (n_rec) {
        HIP_TRY(hipMemcpyAsync(s->h_rows, s->d_rows, n_rec * p->row_bytes, hipMemcpyDeviceToHost, s->stream));
        HIP_TRY(hipMemcpyAsync(s->h_af, s->d_af, n_rec * sizeof(double), hipMemcpyDeviceToHost, s->stream));
        HIP_TRY(hipMemcpyAsync(s->h_het, s->d_het, n_rec * sizeof(unsigned), hipMemcpyDeviceToHost, s->stream));
        HIP_TRY(hipMemcpyAsync(s->h_hom, s->d_hom, n_rec * sizeof(unsigned), hipMemcpyDeviceToHost, s->stream));
        HIP_TRY(hipMemcpyAsync(s->h_status, s->d_status, n_rec * sizeof(unsigned), hipMemcpyDeviceToHost, s->stream));
    }
    HIP_TRY(hipMemcpyAsync(s->h_misc, s->d_misc, 2 * sizeof(unsigned), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipEventRecord(s->ev[5], s->stream));
    s->n_rec = n_rec;
    p->queued();
    return UTM_OK;
}

// The end of both VCF parse calls, once the text of m bytes and its newline counts per block are on the device: the
// records are parsed and copied back, and the batch is queued.
static int vcf_parse_records(utm_vcf *p, VcfSlot *s, u64 m, u64 n_blk, u64 n_rec)
{
    TRY(s->d_nl.reserve(n_rec, 1024));
    TRY(vcf_reserve_results(p, s, n_rec));
    HIP_TRY(hipEventRecord(s->ev[3], s->stream));
    if (n_rec) {
        k_vcf_nl_write<<<(unsigned)n_blk, VCF_THREADS, 0, s->stream>>>(s->d_text, (unsigned)m, s->d_blk, s->d_nl);
        k_vcf_parse<<<(unsigned)n_rec, VCF_THREADS, p->row_words * sizeof(unsigned), s->stream>>>(
            s->d_text, s->d_nl, p->n_samples, p->row_words, p->row_bytes, s->d_rows, s->d_af, s->d_het, s->d_hom, s->d_status, s->d_misc);
        HIP_TRY(hipGetLastError());
    }
    return vcf_results_back(p, s, n_rec);
}

// ... and of the BCF parse call: the record offsets of k_bcf_chain are in d_nl.
static int bcf_parse_records(utm_vcf *p, VcfSlot *s, u64 n, u64 n_rec, unsigned gt_key)
{
    TRY(vcf_reserve_results(p, s, n_rec));
    HIP_TRY(hipEventRecord(s->ev[3], s->stream));
    if (n_rec) {
        k_bcf_parse<<<(unsigned)n_rec, VCF_THREADS, p->row_words * sizeof(unsigned), s->stream>>>(
            s->d_text, s->d_nl, (unsigned)n, p->n_samples, p->row_words, p->row_bytes, gt_key, s->d_rows, s->d_af, s->d_het, s->d_hom,
            s->d_status, s->d_misc);
        HIP_TRY(hipGetLastError());
    }
    return vcf_results_back(p, s, n_rec);
}

extern "C" int utm_vcf_parse(utm_vcf *p, const uint8_t *text, uint64_t n_bytes, uint64_t *n_records)
{
    BATCH_CTX(p, "vcf");
    if (!text || !n_records) return fail(UTM_EINVAL, "text or n_records is NULL");
    if (n_bytes == 0 || n_bytes > UTM_VCF_MAX_BATCH) return fail(UTM_EINVAL, "a batch of %llu bytes (1 .. 2^32 - 64)", (unsigned long long)n_bytes);
    if (text[n_bytes - 1] != '\n') return fail(UTM_EINVAL, "the batch does not end with a newline");
    VcfSlot *s;
    TRY(p->free_slot("utm_vcf_fetch", &s));
    TRY(vcf_slot_ready(p, s));
    p->carry = 0;
    s->bgzf = false;
    if (text != s->h_text) {
        TRY(s->h_text.grow(n_bytes));
        memcpy(s->h_text, text, n_bytes);
    }
    const u64 n_blk = (n_bytes + VCF_BLOCK_BYTES - 1) / VCF_BLOCK_BYTES;
    TRY(s->d_text.reserve(n_bytes + VCF_TEXT_PAD, s->h_text.cap + VCF_TEXT_PAD));
    TRY(s->d_blk.reserve(n_blk));
    const unsigned n = (unsigned)n_bytes;
    HIP_TRY(hipEventRecord(s->ev[0], s->stream));
    HIP_TRY(hipMemcpyAsync(s->d_text, s->h_text, n_bytes, hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipEventRecord(s->ev[1], s->stream));
    k_vcf_nl_count<<<(unsigned)n_blk, VCF_THREADS, 0, s->stream>>>(s->d_text, n, s->d_blk);
    k_vcf_nl_scan<<<1, VCF_THREADS, 0, s->stream>>>(s->d_blk, (unsigned)n_blk, s->d_misc);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(s->ev[2], s->stream));
    HIP_TRY(hipMemcpyAsync(s->h_misc, s->d_misc, 2 * sizeof(unsigned), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));  // the record count sizes everything below (and the staging is free again)
    TRY(vcf_parse_records(p, s, n_bytes, n_blk, s->h_misc[0]));
    *n_records = s->n_rec;
    return UTM_OK;
}

extern "C" int utm_vcf_fetch(utm_vcf *p, uint8_t *rows, double *af, uint32_t *n_het, uint32_t *n_hom, uint8_t *flags)
{
    BATCH_CTX(p, "vcf");
    VcfSlot *s;
    TRY(p->take_oldest("fetch", &s));
    HIP_TRY(hipStreamSynchronize(s->stream));
    if (s->bgzf) {
        TRY(add_elapsed(&p->ms[0], s->ev[0], s->ev_h2d));
        TRY(add_elapsed(&p->inflate_ms, s->ev_h2d, s->ev[1]));
    } else {
        TRY(add_elapsed(&p->ms[0], s->ev[0], s->ev[1]));
    }
    TRY(add_elapsed(&p->find_ms, s->ev[1], s->ev[2]));
    TRY(add_elapsed(&p->parse_ms, s->ev[3], s->ev[4]));
    p->ms[1] = p->find_ms + p->parse_ms;
    TRY(add_elapsed(&p->ms[2], s->ev[4], s->ev[5]));
    const u64 n = s->n_rec;
    if (s->h_misc[1] != 0xFFFFFFFFu) {
        const unsigned r = s->h_misc[1];
        return fail(UTM_EINVAL, "record %u of the batch: %s", r, vcf_error_text(s->h_status[r] >> 8));
    }
    if (!n) return UTM_OK;
    if (!rows || !af || !n_het || !n_hom || !flags) return fail(UTM_EINVAL, "output is NULL");
    memcpy(rows, s->h_rows, n * p->row_bytes);
    memcpy(af, s->h_af, n * sizeof(double));
    memcpy(n_het, s->h_het, n * sizeof(unsigned));
    memcpy(n_hom, s->h_hom, n * sizeof(unsigned));
    for (u64 i = 0; i < n; ++i) flags[i] = (uint8_t)(s->h_status[i] & 0xFF);
    return UTM_OK;
}

extern "C" int utm_vcf_timing(utm_vcf *p, double *ms)
{
    if (!p || !ms) return fail(UTM_EINVAL, "vcf or ms is NULL");
    for (int i = 0; i < 3; ++i) ms[i] = p->ms[i];
    return UTM_OK;
}

// The member table of a BGZF batch: compressed bytes back to back in the staging, text from *out on; *out = its end.
static int vcf_member_table(VcfSlot *s, const uint32_t *members, u64 n_members, u64 packed_bytes, u64 *out)
{
    u64 in_off = 0;
    for (u64 i = 0; i < n_members; ++i) {
        const u64 in_size = members[2 * i], isize = members[2 * i + 1];
        if (in_size > packed_bytes - in_off) return fail(UTM_EINVAL, "member %llu runs past the %llu compressed bytes", (unsigned long long)i, (unsigned long long)packed_bytes);
        if (isize > INF_OUT_MAX) return fail(UTM_EINVAL, "member %llu of the batch: %s", (unsigned long long)i, inf_error_text(INF_E_ISIZE));
        s->h_members[i] = InfMember{(unsigned)in_off, (unsigned)in_size, (unsigned)*out, (unsigned)isize};
        in_off += in_size;
        *out += isize;
        if (*out + 1 > UTM_VCF_MAX_BATCH) return fail(UTM_EINVAL, "a batch of more than 2^32 - 64 text bytes");
    }
    if (in_off != packed_bytes) return fail(UTM_EINVAL, "the members hold %llu of the %llu compressed bytes", (unsigned long long)in_off, (unsigned long long)packed_bytes);
    return UTM_OK;
}

// Member i of the batch failed on the device: its status word becomes the call's error.
static int vcf_member_failure(VcfSlot *s, unsigned i)
{
    unsigned st = 0;
    HIP_TRY(hipMemcpy(&st, s->d_mstat + i, sizeof st, hipMemcpyDeviceToHost));
    const unsigned code = st & 255, got = st >> 8, isize = s->h_members[i].isize;
    if (code == INF_E_LENGTH) return fail(UTM_EINVAL, "member %u of the batch: %u bytes inflated, ISIZE says %u", i, got, isize);
    if (code == INF_E_OUTPUT) return fail(UTM_EINVAL, "member %u of the batch: more than %u bytes inflated, ISIZE says %u", i, isize, isize);
    return fail(UTM_EINVAL, "member %u of the batch: %s", i, inf_error_text(code));
}

extern "C" int utm_vcf_parse_bgzf(utm_vcf *p, const uint8_t *prefix, uint64_t prefix_bytes, const uint8_t *packed,
                                  uint64_t packed_bytes, const uint32_t *members, uint64_t n_members, uint32_t flags,
                                  uint64_t *n_records, uint64_t *carry_bytes)
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
    // the member table: compressed bytes back to back in `packed`, text after the carry and the prefix
    if (packed_bytes > UTM_VCF_MAX_BATCH) return fail(UTM_EINVAL, "a batch of %llu compressed bytes (at most 2^32 - 64)", (unsigned long long)packed_bytes);
    TRY(s->d_packed.reserve(packed_bytes, s->h_text.cap));
    TRY(s->d_members.reserve(n_members, 1024));
    TRY(s->d_mstat.reserve(n_members, 1024));
    TRY(s->h_members.reserve(n_members, 1024));
    u64 out = carry + prefix_bytes;
    TRY(vcf_member_table(s, members, n_members, packed_bytes, &out));
    const u64 n = out, m = n + (last ? 1 : 0);  // m: the text the parser sees (the last batch: + '\n' or a 0)
    if (packed && packed != s->h_text && packed_bytes) {
        TRY(s->h_text.grow(packed_bytes));
        memcpy(s->h_text, packed, packed_bytes);
    }
    TRY(vcf_slot_ready(p, s));
    TRY(s->d_text.grow(m + VCF_TEXT_PAD, carry, s->stream));
    const u64 n_blk = std::max<u64>(1, (m + VCF_BLOCK_BYTES - 1) / VCF_BLOCK_BYTES);
    TRY(s->d_blk.reserve(n_blk));
    s->bgzf = true;
    HIP_TRY(hipEventRecord(s->ev[0], s->stream));
    if (packed_bytes) HIP_TRY(hipMemcpyAsync(s->d_packed, s->h_text, packed_bytes, hipMemcpyHostToDevice, s->stream));
    if (n_members) HIP_TRY(hipMemcpyAsync(s->d_members, s->h_members, n_members * sizeof(InfMember), hipMemcpyHostToDevice, s->stream));
    if (prefix_bytes) HIP_TRY(hipMemcpyAsync(s->d_text + carry, prefix, prefix_bytes, hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipEventRecord(s->ev_h2d, s->stream));
    // misc: [0] records, [1] first failing record, [2] 1 + last newline, [3] first failing member
    HIP_TRY(hipMemsetAsync(s->d_misc, 0, 4 * sizeof(unsigned), s->stream));
    HIP_TRY(hipMemsetAsync(s->d_misc + 1, 0xFF, sizeof(unsigned), s->stream));
    HIP_TRY(hipMemsetAsync(s->d_misc + 3, 0xFF, sizeof(unsigned), s->stream));
    if (n_members) k_bgzf_inflate<<<(unsigned)n_members, INF_THREADS, 0, s->stream>>>(s->d_packed, s->d_members, s->d_text, s->d_mstat, s->d_misc);
    if (last) k_bgzf_finish<<<1, 64, 0, s->stream>>>(s->d_text, (unsigned)n);
    if (m) k_bgzf_last_nl<<<(unsigned)n_blk, VCF_THREADS, 0, s->stream>>>(s->d_text, (unsigned)m, s->d_misc);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(s->ev[1], s->stream));
    if (m) {
        k_vcf_nl_count<<<(unsigned)n_blk, VCF_THREADS, 0, s->stream>>>(s->d_text, (unsigned)m, s->d_blk);
        k_vcf_nl_scan<<<1, VCF_THREADS, 0, s->stream>>>(s->d_blk, (unsigned)n_blk, s->d_misc);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(s->ev[2], s->stream));
    HIP_TRY(hipMemcpyAsync(s->h_misc, s->d_misc, 4 * sizeof(unsigned), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));  // records, carry, the first failing member
    if (s->h_misc[3] != 0xFFFFFFFFu) return vcf_member_failure(s, s->h_misc[3]);
    const u64 n_rec = m ? s->h_misc[0] : 0, cut = s->h_misc[2];
    const u64 carry_next = last ? 0 : m - cut;
    if (carry_next) {  // the unfinished record: to the head of the other slot's text, on that slot's stream
        VcfSlot *o = p->other(s);
        TRY(o->d_text.grow(carry_next + VCF_TEXT_PAD, 0, o->stream));
        HIP_TRY(hipEventRecord(s->ev[3], s->stream));
        HIP_TRY(hipStreamWaitEvent(o->stream, s->ev[3], 0));
        HIP_TRY(hipMemcpyAsync(o->d_text, s->d_text + cut, carry_next, hipMemcpyDeviceToDevice, o->stream));
        HIP_TRY(hipEventRecord(o->ev_carry, o->stream));
        s->carry_out = true;
    }
    TRY(vcf_parse_records(p, s, m, n_blk, n_rec));
    p->carry = carry_next;
    *n_records = n_rec;
    *carry_bytes = carry_next;
    return UTM_OK;
}

extern "C" int utm_vcf_kernel_timing(utm_vcf *p, double *ms)
{
    if (!p || !ms) return fail(UTM_EINVAL, "vcf or ms is NULL");
    ms[0] = p->find_ms;
    ms[1] = p->parse_ms;
    return UTM_OK;
}

extern "C" int utm_vcf_inflate_timing(utm_vcf *p, double *ms)
{
    if (!p || !ms) return fail(UTM_EINVAL, "vcf or ms is NULL");
    ms[0] = p->inflate_ms;
    return UTM_OK;
}

// The decoder of k_bgzf_inflate built for the CPU (one lane): tests and tools check it against zlib without a GPU.
extern "C" int utm_bgzf_inflate_host(const uint8_t *member, uint64_t member_bytes, uint8_t *out, uint64_t out_cap,
                                     uint32_t *status)
{
    if (!status || (member_bytes && !member) || (out_cap && !out)) return fail(UTM_EINVAL, "member, out or status is NULL");
    if (member_bytes > 0xFFFFFFFFull) return fail(UTM_EINVAL, "a member of %llu bytes", (unsigned long long)member_bytes);
    const uint32_t isize = member_bytes >= 8 ? inf_rd32(member + member_bytes - 4) : 0;
    std::vector<uint8_t> buf(INF_OUT_MAX + 16);
    std::vector<InfTables> t(1);
    const uint32_t st = inf_member(member, (uint32_t)member_bytes, buf.data(), isize, t.data(), 0, 1);
    if (out_cap) memcpy(out, buf.data(), std::min<u64>(out_cap, std::min<u64>(st >> 8, INF_OUT_MAX)));
    *status = st;
    return UTM_OK;
}
