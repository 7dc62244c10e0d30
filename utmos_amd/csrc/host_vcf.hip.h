// VCF parse context (utm_vcf_*): host side of vcf.hip.h and inflate.hip.h.  Restates the genotype half of the
// reference's convert (utmos/convert.py:43-88) for text the caller has already split off its header: inflated on the
// host (utm_vcf_parse) or BGZF members inflated on the device (utm_vcf_parse_bgzf).
//
// Two slots, each with its own stream, pinned staging, device text and per-record buffers: utm_vcf_parse returns once
// its batch has reached the device and the parse is queued, so the caller fills the other slot's staging (inflate,
// read) while the GPU parses; utm_vcf_fetch then collects the oldest batch.
//
// BGZF batches end at member borders, so a record may run from one batch into the next.  The bytes after the last
// newline of a batch (the carry) are copied on the device to the head of the other slot's text, and the next batch
// inflates after them: the host never sees the text.
#pragma once

struct VcfSlot {
    hipStream_t stream = nullptr;
    hipEvent_t ev[6] = {};  // around: H2D (0-1), count + scan (1-2), [host reads the count], write + parse (3-4), D2H (4-5)
    unsigned char *h_text = nullptr, *d_text = nullptr;
    u64 h_cap = 0, d_cap = 0;
    unsigned *d_blk = nullptr;
    u64 blk_cap = 0;
    unsigned *d_misc = nullptr, *h_misc = nullptr;  // [0] records, [1] first failing record
    // per record
    u64 rec_cap = 0;
    unsigned char *d_rows = nullptr;
    unsigned *d_nl = nullptr, *d_het = nullptr, *d_hom = nullptr, *d_status = nullptr;
    double *d_af = nullptr;
    unsigned char *h_rows = nullptr;
    double *h_af = nullptr;
    unsigned *h_het = nullptr, *h_hom = nullptr, *h_status = nullptr;
    u64 n_rec = 0;
    bool pending = false;
    // BGZF batches: compressed bytes and the member table on the device, a status word per member
    unsigned char *d_packed = nullptr;
    u64 packed_cap = 0;
    InfMember *d_members = nullptr, *h_members = nullptr;
    unsigned *d_mstat = nullptr;
    u64 mem_cap = 0;
    hipEvent_t ev_h2d = nullptr;    // BGZF: end of the copies in (ev[0] .. ev_h2d), inflate (ev_h2d .. ev[1])
    hipEvent_t ev_carry = nullptr;  // on this slot's stream: the carry copy into its text is done
    bool bgzf = false;              // the pending batch came through utm_vcf_parse_bgzf
    bool carry_out = false;         // this slot's text is the source of a carry copy on the other stream
};

struct utm_vcf {
    int device = 0;
    uint32_t n_samples = 0;
    uint32_t row_words = 0;  // LDS row in the kernel: ceil(S / 32) words
    uint32_t row_bytes = 0;  // packed row: ceil(S / 8) bytes
    VcfSlot slot[2];
    int next = 0;       // slot of the next utm_vcf_parse
    int oldest = 0;     // slot of the next utm_vcf_fetch
    int n_pending = 0;
    double ms[3] = {0, 0, 0};  // H2D, kernels, D2H
    double inflate_ms = 0;     // BGZF inflate kernels
    u64 carry = 0;             // bytes at the head of slot[next]'s text that the next BGZF batch continues
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

static void vcf_slot_free(VcfSlot *s)
{
    if (s->h_text) (void)hipHostFree(s->h_text);
    if (s->h_misc) (void)hipHostFree(s->h_misc);
    if (s->h_rows) (void)hipHostFree(s->h_rows);
    if (s->h_af) (void)hipHostFree(s->h_af);
    if (s->h_het) (void)hipHostFree(s->h_het);
    if (s->h_hom) (void)hipHostFree(s->h_hom);
    if (s->h_status) (void)hipHostFree(s->h_status);
    if (s->h_members) (void)hipHostFree(s->h_members);
    void *dev[] = {s->d_text, s->d_blk, s->d_misc, s->d_nl, s->d_rows, s->d_het, s->d_hom, s->d_status, s->d_af,
                   s->d_packed, s->d_members, s->d_mstat};
    for (void *d : dev)
        if (d) (void)hipFree(d);
    for (hipEvent_t e : s->ev)
        if (e) (void)hipEventDestroy(e);
    if (s->ev_h2d) (void)hipEventDestroy(s->ev_h2d);
    if (s->ev_carry) (void)hipEventDestroy(s->ev_carry);
    if (s->stream) (void)hipStreamDestroy(s->stream);
    *s = VcfSlot();
}

// Pinned staging of at least n bytes; keeps what it held (a record longer than a batch grows the buffer mid-fill).
static int vcf_grow_staging(VcfSlot *s, u64 n)
{
    if (s->h_cap >= n) return UTM_OK;
    u64 cap = std::max<u64>(n, s->h_cap + s->h_cap / 2);
    unsigned char *p = nullptr;
    HIP_TRY(hipHostMalloc((void **)&p, cap, hipHostMallocDefault));
    if (s->h_text) {
        memcpy(p, s->h_text, s->h_cap);
        (void)hipHostFree(s->h_text);
    }
    s->h_text = p;
    s->h_cap = cap;
    return UTM_OK;
}

static int vcf_grow_device(utm_vcf *p, VcfSlot *s, u64 n_bytes, u64 n_blk, u64 n_rec)
{
    if (s->d_cap < n_bytes) {
        if (s->d_text) (void)hipFree(s->d_text);
        s->d_text = nullptr;
        s->d_cap = 0;
        const u64 cap = std::max<u64>(n_bytes, s->h_cap);
        HIP_TRY(hipMalloc(&s->d_text, cap + 64));  // 16-byte loads may run past the last record
        s->d_cap = cap;
    }
    if (s->blk_cap < n_blk) {
        if (s->d_blk) (void)hipFree(s->d_blk);
        s->d_blk = nullptr;
        s->blk_cap = 0;
        HIP_TRY(hipMalloc(&s->d_blk, n_blk * sizeof(unsigned)));
        s->blk_cap = n_blk;
    }
    if (s->rec_cap < n_rec) {
        void *dev[] = {s->d_nl, s->d_rows, s->d_het, s->d_hom, s->d_status, s->d_af};
        for (void *d : dev)
            if (d) (void)hipFree(d);
        void *host[] = {s->h_rows, s->h_af, s->h_het, s->h_hom, s->h_status};
        for (void *h : host)
            if (h) (void)hipHostFree(h);
        s->d_rows = nullptr;
        s->d_nl = s->d_het = s->d_hom = s->d_status = nullptr;
        s->d_af = nullptr;
        s->h_rows = nullptr;
        s->h_af = nullptr;
        s->h_het = s->h_hom = s->h_status = nullptr;
        s->rec_cap = 0;
        const u64 cap = std::max<u64>(n_rec, 1024);
        HIP_TRY(hipMalloc(&s->d_nl, cap * sizeof(unsigned)));
        HIP_TRY(hipMalloc(&s->d_rows, cap * p->row_bytes));
        HIP_TRY(hipMalloc(&s->d_het, cap * sizeof(unsigned)));
        HIP_TRY(hipMalloc(&s->d_hom, cap * sizeof(unsigned)));
        HIP_TRY(hipMalloc(&s->d_status, cap * sizeof(unsigned)));
        HIP_TRY(hipMalloc(&s->d_af, cap * sizeof(double)));
        HIP_TRY(hipHostMalloc((void **)&s->h_rows, cap * p->row_bytes, hipHostMallocDefault));
        HIP_TRY(hipHostMalloc((void **)&s->h_af, cap * sizeof(double), hipHostMallocDefault));
        HIP_TRY(hipHostMalloc((void **)&s->h_het, cap * sizeof(unsigned), hipHostMallocDefault));
        HIP_TRY(hipHostMalloc((void **)&s->h_hom, cap * sizeof(unsigned), hipHostMallocDefault));
        HIP_TRY(hipHostMalloc((void **)&s->h_status, cap * sizeof(unsigned), hipHostMallocDefault));
        s->rec_cap = cap;
    }
    return UTM_OK;
}

// The slot's text may be written once a carry copy out of it (queued on the other slot's stream) is done.
static int vcf_slot_ready(utm_vcf *p, VcfSlot *s)
{
    if (s->carry_out) {
        HIP_TRY(hipStreamWaitEvent(s->stream, p->slot[s == &p->slot[0]].ev_carry, 0));
        s->carry_out = false;
    }
    return UTM_OK;
}

#define VCF(p)                                       \
    if (!(p)) return fail(UTM_EINVAL, "vcf is NULL"); \
    HIP_TRY(hipSetDevice((p)->device))

extern "C" int utm_vcf_create(int device, uint32_t n_samples, uint64_t batch_bytes, utm_vcf **out)
{
    if (!out) return fail(UTM_EINVAL, "out is NULL");
    *out = nullptr;
    if (n_samples == 0 || n_samples > UTM_VCF_MAX_SAMPLES)
        return fail(UTM_EINVAL, "n_samples %u not in [1, %u]", n_samples, (unsigned)UTM_VCF_MAX_SAMPLES);
    if (batch_bytes == 0 || batch_bytes > UTM_VCF_MAX_BATCH) return fail(UTM_EINVAL, "batch_bytes %llu not in [1, 2^32 - 64)", (unsigned long long)batch_bytes);
    int n = 0;
    HIP_TRY(hipGetDeviceCount(&n));
    if (device < 0 || device >= n) return fail(UTM_EINVAL, "device %d of %d", device, n);
    HIP_TRY(hipSetDevice(device));
    if (n_samples > 32768u * 8u)  // rows above 32 KiB of LDS ask for it explicitly
        HIP_TRY(hipFuncSetAttribute((const void *)k_vcf_parse, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)(((n_samples + 31) / 32) * sizeof(unsigned))));
    utm_vcf *p = new utm_vcf();
    p->device = device;
    p->n_samples = n_samples;
    p->row_words = (n_samples + 31) / 32;
    p->row_bytes = (n_samples + 7) / 8;
    int rc = UTM_OK;
    for (VcfSlot &s : p->slot) {
        hipError_t e = hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking);
        for (hipEvent_t &ev : s.ev)
            if (e == hipSuccess) e = hipEventCreate(&ev);
        if (e == hipSuccess) e = hipEventCreate(&s.ev_h2d);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&s.ev_carry, hipEventDisableTiming);
        if (e == hipSuccess) e = hipMalloc(&s.d_misc, 4 * sizeof(unsigned));
        if (e == hipSuccess) e = hipHostMalloc((void **)&s.h_misc, 4 * sizeof(unsigned), hipHostMallocDefault);
        if (e != hipSuccess) rc = fail(e == hipErrorOutOfMemory ? UTM_ENOMEM : UTM_EHIP, "utm_vcf_create: %s", hipGetErrorString(e));
        if (rc == UTM_OK) rc = vcf_grow_staging(&s, batch_bytes);
        if (rc == UTM_OK) rc = vcf_grow_device(p, &s, batch_bytes, (batch_bytes + VCF_BLOCK_BYTES - 1) / VCF_BLOCK_BYTES, 0);
        if (rc != UTM_OK) break;
    }
    if (rc != UTM_OK) {
        for (VcfSlot &s : p->slot) vcf_slot_free(&s);
        delete p;
        return rc;
    }
    *out = p;
    return UTM_OK;
}

extern "C" int utm_vcf_destroy(utm_vcf *p)
{
    if (!p) return UTM_OK;
    (void)hipSetDevice(p->device);
    for (VcfSlot &s : p->slot) {
        if (s.stream) (void)hipStreamSynchronize(s.stream);
        vcf_slot_free(&s);
    }
    delete p;
    return UTM_OK;
}

extern "C" int utm_vcf_staging(utm_vcf *p, uint64_t n_bytes, uint8_t **buf, uint64_t *cap)
{
    VCF(p);
    if (!buf || !cap) return fail(UTM_EINVAL, "output is NULL");
    if (n_bytes > UTM_VCF_MAX_BATCH) return fail(UTM_EINVAL, "a batch of %llu bytes (at most 2^32 - 64)", (unsigned long long)n_bytes);
    VcfSlot *s = &p->slot[p->next];
    TRY(vcf_grow_staging(s, n_bytes));
    *buf = s->h_text;
    *cap = s->h_cap;
    return UTM_OK;
}

extern "C" int utm_vcf_parse(utm_vcf *p, const uint8_t *text, uint64_t n_bytes, uint64_t *n_records)
{
    VCF(p);
    if (!text || !n_records) return fail(UTM_EINVAL, "text or n_records is NULL");
    if (n_bytes == 0 || n_bytes > UTM_VCF_MAX_BATCH) return fail(UTM_EINVAL, "a batch of %llu bytes (1 .. 2^32 - 64)", (unsigned long long)n_bytes);
    if (text[n_bytes - 1] != '\n') return fail(UTM_EINVAL, "the batch does not end with a newline");
    VcfSlot *s = &p->slot[p->next];
    if (s->pending) return fail(UTM_ESTATE, "both slots hold a batch: utm_vcf_fetch first");
    TRY(vcf_slot_ready(p, s));
    p->carry = 0;
    s->bgzf = false;
    if (text != s->h_text) {
        TRY(vcf_grow_staging(s, n_bytes));
        memcpy(s->h_text, text, n_bytes);
    }
    const u64 n_blk = (n_bytes + VCF_BLOCK_BYTES - 1) / VCF_BLOCK_BYTES;
    TRY(vcf_grow_device(p, s, n_bytes, n_blk, 0));
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
    const u64 n_rec = s->h_misc[0];
    TRY(vcf_grow_device(p, s, n_bytes, n_blk, n_rec));
    HIP_TRY(hipEventRecord(s->ev[3], s->stream));
    k_vcf_nl_write<<<(unsigned)n_blk, VCF_THREADS, 0, s->stream>>>(s->d_text, n, s->d_blk, s->d_nl);
    if (n_rec)
        k_vcf_parse<<<(unsigned)n_rec, VCF_THREADS, p->row_words * sizeof(unsigned), s->stream>>>(
            s->d_text, s->d_nl, p->n_samples, p->row_words, p->row_bytes, s->d_rows, s->d_af, s->d_het, s->d_hom, s->d_status, s->d_misc);
    HIP_TRY(hipGetLastError());
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
    s->pending = true;
    p->next ^= 1;
    ++p->n_pending;
    *n_records = n_rec;
    return UTM_OK;
}

extern "C" int utm_vcf_fetch(utm_vcf *p, uint8_t *rows, double *af, uint32_t *n_het, uint32_t *n_hom, uint8_t *flags)
{
    VCF(p);
    if (!p->n_pending) return fail(UTM_ESTATE, "no batch to fetch");
    VcfSlot *s = &p->slot[p->oldest];
    // the slot is released on every way out, so a failed batch leaves the context usable
    s->pending = false;
    p->oldest ^= 1;
    --p->n_pending;
    HIP_TRY(hipStreamSynchronize(s->stream));
    float a = 0, b = 0, c = 0, d = 0;
    if (s->bgzf) {
        float f = 0;
        HIP_TRY(hipEventElapsedTime(&a, s->ev[0], s->ev_h2d));
        HIP_TRY(hipEventElapsedTime(&f, s->ev_h2d, s->ev[1]));
        p->inflate_ms += f;
    } else {
        HIP_TRY(hipEventElapsedTime(&a, s->ev[0], s->ev[1]));
    }
    HIP_TRY(hipEventElapsedTime(&b, s->ev[1], s->ev[2]));
    HIP_TRY(hipEventElapsedTime(&c, s->ev[3], s->ev[4]));
    HIP_TRY(hipEventElapsedTime(&d, s->ev[4], s->ev[5]));
    p->ms[0] += a;
    p->ms[1] += b + c;
    p->ms[2] += d;
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

// Device text of at least n bytes (+ 64 readable past the end) that keeps its first `keep` bytes (the carry).
static int vcf_grow_text(VcfSlot *s, u64 n, u64 keep)
{
    if (s->d_cap >= n) return UTM_OK;
    HIP_TRY(hipStreamSynchronize(s->stream));  // the old text is neither read nor written any more
    const u64 cap = std::max<u64>(n, s->d_cap + s->d_cap / 2);
    unsigned char *d = nullptr;
    HIP_TRY(hipMalloc(&d, cap + 64));
    if (keep) {
        hipError_t e = hipMemcpy(d, s->d_text, keep, hipMemcpyDeviceToDevice);
        if (e != hipSuccess) {
            (void)hipFree(d);
            return fail(UTM_EHIP, "carry copy: %s", hipGetErrorString(e));
        }
    }
    if (s->d_text) (void)hipFree(s->d_text);
    s->d_text = d;
    s->d_cap = cap;
    return UTM_OK;
}

static int vcf_grow_bgzf(VcfSlot *s, u64 packed_bytes, u64 n_members)
{
    if (s->packed_cap < packed_bytes) {
        if (s->d_packed) (void)hipFree(s->d_packed);
        s->d_packed = nullptr;
        s->packed_cap = 0;
        const u64 cap = std::max<u64>(packed_bytes, s->h_cap);
        HIP_TRY(hipMalloc(&s->d_packed, cap));
        s->packed_cap = cap;
    }
    if (s->mem_cap < n_members) {
        if (s->d_members) (void)hipFree(s->d_members);
        if (s->d_mstat) (void)hipFree(s->d_mstat);
        if (s->h_members) (void)hipHostFree(s->h_members);
        s->d_members = s->h_members = nullptr;
        s->d_mstat = nullptr;
        s->mem_cap = 0;
        const u64 cap = std::max<u64>(n_members, 1024);
        HIP_TRY(hipMalloc(&s->d_members, cap * sizeof(InfMember)));
        HIP_TRY(hipMalloc(&s->d_mstat, cap * sizeof(unsigned)));
        HIP_TRY(hipHostMalloc((void **)&s->h_members, cap * sizeof(InfMember), hipHostMallocDefault));
        s->mem_cap = cap;
    }
    return UTM_OK;
}

extern "C" int utm_vcf_parse_bgzf(utm_vcf *p, const uint8_t *prefix, uint64_t prefix_bytes, const uint8_t *packed,
                                  uint64_t packed_bytes, const uint32_t *members, uint64_t n_members, uint32_t flags,
                                  uint64_t *n_records, uint64_t *carry_bytes)
{
    VCF(p);
    if (!n_records || !carry_bytes) return fail(UTM_EINVAL, "n_records or carry_bytes is NULL");
    if ((prefix_bytes && !prefix) || (packed_bytes && !packed) || (n_members && !members))
        return fail(UTM_EINVAL, "prefix, packed or members is NULL");
    if (flags & ~(UTM_BGZF_FIRST | UTM_BGZF_LAST)) return fail(UTM_EINVAL, "unknown flags 0x%x", flags);
    VcfSlot *s = &p->slot[p->next];
    if (s->pending) return fail(UTM_ESTATE, "both slots hold a batch: utm_vcf_fetch first");
    if (flags & UTM_BGZF_FIRST) p->carry = 0;
    const bool last = flags & UTM_BGZF_LAST;
    const u64 carry = p->carry;
    p->carry = 0;  // (set again once this batch has succeeded)
    // the member table: compressed bytes back to back in `packed`, text after the carry and the prefix
    if (packed_bytes > UTM_VCF_MAX_BATCH) return fail(UTM_EINVAL, "a batch of %llu compressed bytes (at most 2^32 - 64)", (unsigned long long)packed_bytes);
    TRY(vcf_grow_bgzf(s, packed_bytes, n_members));
    u64 in_off = 0, out = carry + prefix_bytes;
    for (u64 i = 0; i < n_members; ++i) {
        const u64 in_size = members[2 * i], isize = members[2 * i + 1];
        if (in_size > packed_bytes - in_off) return fail(UTM_EINVAL, "member %llu runs past the %llu compressed bytes", (unsigned long long)i, (unsigned long long)packed_bytes);
        if (isize > INF_OUT_MAX) return fail(UTM_EINVAL, "member %llu of the batch: %s", (unsigned long long)i, inf_error_text(INF_E_ISIZE));
        s->h_members[i] = InfMember{(unsigned)in_off, (unsigned)in_size, (unsigned)out, (unsigned)isize};
        in_off += in_size;
        out += isize;
        if (out + 1 > UTM_VCF_MAX_BATCH) return fail(UTM_EINVAL, "a batch of more than 2^32 - 64 text bytes");
    }
    if (in_off != packed_bytes) return fail(UTM_EINVAL, "the members hold %llu of the %llu compressed bytes", (unsigned long long)in_off, (unsigned long long)packed_bytes);
    const u64 n = out, m = n + (last ? 1 : 0);  // m: the text the parser sees (the last batch: + '\n' or a 0)
    if (packed && packed != s->h_text && packed_bytes) {
        TRY(vcf_grow_staging(s, packed_bytes));
        memcpy(s->h_text, packed, packed_bytes);
    }
    TRY(vcf_slot_ready(p, s));
    TRY(vcf_grow_text(s, m, carry));
    const u64 n_blk = std::max<u64>(1, (m + VCF_BLOCK_BYTES - 1) / VCF_BLOCK_BYTES);
    TRY(vcf_grow_device(p, s, m, n_blk, 0));
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
    if (s->h_misc[3] != 0xFFFFFFFFu) {
        const unsigned i = s->h_misc[3];
        unsigned st = 0;
        HIP_TRY(hipMemcpy(&st, s->d_mstat + i, sizeof st, hipMemcpyDeviceToHost));
        const unsigned code = st & 255, got = st >> 8, isize = s->h_members[i].isize;
        if (code == INF_E_LENGTH) return fail(UTM_EINVAL, "member %u of the batch: %u bytes inflated, ISIZE says %u", i, got, isize);
        if (code == INF_E_OUTPUT) return fail(UTM_EINVAL, "member %u of the batch: more than %u bytes inflated, ISIZE says %u", i, isize, isize);
        return fail(UTM_EINVAL, "member %u of the batch: %s", i, inf_error_text(code));
    }
    const u64 n_rec = m ? s->h_misc[0] : 0, cut = s->h_misc[2];
    const u64 carry_next = last ? 0 : m - cut;
    if (carry_next) {  // the unfinished record: to the head of the other slot's text, on that slot's stream
        VcfSlot *o = &p->slot[p->next ^ 1];
        TRY(vcf_grow_text(o, carry_next, 0));
        HIP_TRY(hipEventRecord(s->ev[3], s->stream));
        HIP_TRY(hipStreamWaitEvent(o->stream, s->ev[3], 0));
        HIP_TRY(hipMemcpyAsync(o->d_text, s->d_text + cut, carry_next, hipMemcpyDeviceToDevice, o->stream));
        HIP_TRY(hipEventRecord(o->ev_carry, o->stream));
        s->carry_out = true;
    }
    TRY(vcf_grow_device(p, s, m, n_blk, n_rec));
    HIP_TRY(hipEventRecord(s->ev[3], s->stream));
    if (n_rec) {
        k_vcf_nl_write<<<(unsigned)n_blk, VCF_THREADS, 0, s->stream>>>(s->d_text, (unsigned)m, s->d_blk, s->d_nl);
        k_vcf_parse<<<(unsigned)n_rec, VCF_THREADS, p->row_words * sizeof(unsigned), s->stream>>>(
            s->d_text, s->d_nl, p->n_samples, p->row_words, p->row_bytes, s->d_rows, s->d_af, s->d_het, s->d_hom, s->d_status, s->d_misc);
        HIP_TRY(hipGetLastError());
    }
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
    s->pending = true;
    p->next ^= 1;
    ++p->n_pending;
    p->carry = carry_next;
    *n_records = n_rec;
    *carry_bytes = carry_next;
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
