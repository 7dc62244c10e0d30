// VCF parse context (utm_vcf_*): host side of vcf.hip.h.  Restates the genotype half of the reference's convert
// (utmos/convert.py:43-88) for text the caller has already split off its header and inflated.
//
// Two slots, each with its own stream, pinned staging, device text and per-record buffers: utm_vcf_parse returns once
// its batch has reached the device and the parse is queued, so the caller fills the other slot's staging (inflate,
// read) while the GPU parses; utm_vcf_fetch then collects the oldest batch.
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

static void vcf_slot_free(VcfSlot *s)
{
    if (s->h_text) (void)hipHostFree(s->h_text);
    if (s->h_misc) (void)hipHostFree(s->h_misc);
    if (s->h_rows) (void)hipHostFree(s->h_rows);
    if (s->h_af) (void)hipHostFree(s->h_af);
    if (s->h_het) (void)hipHostFree(s->h_het);
    if (s->h_hom) (void)hipHostFree(s->h_hom);
    if (s->h_status) (void)hipHostFree(s->h_status);
    void *dev[] = {s->d_text, s->d_blk, s->d_misc, s->d_nl, s->d_rows, s->d_het, s->d_hom, s->d_status, s->d_af};
    for (void *d : dev)
        if (d) (void)hipFree(d);
    for (hipEvent_t e : s->ev)
        if (e) (void)hipEventDestroy(e);
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
        if (e == hipSuccess) e = hipMalloc(&s.d_misc, 2 * sizeof(unsigned));
        if (e == hipSuccess) e = hipHostMalloc((void **)&s.h_misc, 2 * sizeof(unsigned), hipHostMallocDefault);
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
    HIP_TRY(hipEventElapsedTime(&a, s->ev[0], s->ev[1]));
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
