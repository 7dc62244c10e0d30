// The two-slot batch pipeline of the codec contexts (host_vcf, host_deflate, host_h5).  A submit call queues a batch on
// the free slot and returns once the caller may refill its staging; a fetch (pull) call waits for the oldest slot.
// Each slot owns a stream, timing events and its buffers (Scratch on the device, Pinned on the host).
//
// Lifetime: a context's destructor sets its device and waits for both streams (SlotPair::idle) before any buffer goes,
// since work queued on one slot's stream may read the other slot's memory (the VCF carry copy).  Members are destroyed
// after the destructor's body, so the wait cannot sit in a slot's own destructor.
#pragma once

#include <memory>

// Pinned host memory, the mirror of Scratch.
template <typename T>
struct Pinned {
    T *p = nullptr;
    u64 cap = 0;  // elements
    Pinned() = default;
    Pinned(const Pinned &) = delete;
    Pinned &operator=(const Pinned &) = delete;
    ~Pinned() { if (p) (void)hipHostFree(p); }
    // Room for at least `count` elements (`floor` of them when it has to grow and that is more); drops the contents.
    int reserve(u64 count, u64 floor = 0)
    {
        if (cap >= count) return UTM_OK;
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
        HIP_TRY(hipHostMalloc((void **)&p, std::max(count, floor) * sizeof(T), hipHostMallocDefault));
        cap = std::max(count, floor);
        return UTM_OK;
    }
    // Room for at least `count` elements, growing by half at least; keeps the contents.
    int grow(u64 count)
    {
        if (cap >= count) return UTM_OK;
        const u64 n = std::max(count, cap + cap / 2);
        T *q = nullptr;
        HIP_TRY(hipHostMalloc((void **)&q, n * sizeof(T), hipHostMallocDefault));
        if (p) memcpy(q, p, cap * sizeof(T));
        if (p) (void)hipHostFree(p);
        p = q;
        cap = n;
        return UTM_OK;
    }
    operator T *() const { return p; }
};

template <int N_EV>
struct BatchSlot {
    hipStream_t stream = nullptr;
    hipEvent_t ev[N_EV] = {};
    bool pending = false;  // holds a batch that is not fetched yet
    BatchSlot() = default;
    BatchSlot(const BatchSlot &) = delete;
    BatchSlot &operator=(const BatchSlot &) = delete;
    ~BatchSlot()
    {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
        if (stream) (void)hipStreamDestroy(stream);
    }
    int open()
    {
        HIP_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        for (hipEvent_t &e : ev) HIP_TRY(hipEventCreate(&e));
        return UTM_OK;
    }
};

template <typename Slot>
struct SlotPair {
    Slot slot[2];
    int next = 0;    // slot of the next submit
    int oldest = 0;  // slot of the next fetch
    int n_pending = 0;

    Slot *next_slot() { return &slot[next]; }
    Slot *other(const Slot *s) { return &slot[s == &slot[0]]; }
    // The slot of the next submit, when it is free; `fetch` names the call that frees one.
    int free_slot(const char *fetch, Slot **out)
    {
        if (slot[next].pending) return fail(UTM_ESTATE, "both slots hold a batch: %s first", fetch);
        *out = &slot[next];
        return UTM_OK;
    }
    // The batch on the free slot is queued.
    void queued()
    {
        slot[next].pending = true;
        next ^= 1;
        ++n_pending;
    }
    // The oldest batch's slot, or null when there is none.
    Slot *peek_oldest() { return n_pending ? &slot[oldest] : nullptr; }
    // ... released at once, so every way out of the fetch leaves the context usable.
    int take_oldest(const char *verb, Slot **out)
    {
        if (!n_pending) return fail(UTM_ESTATE, "no batch to %s", verb);
        *out = &slot[oldest];
        slot[oldest].pending = false;
        oldest ^= 1;
        --n_pending;
        return UTM_OK;
    }
    // The first thing a context's destructor does (see the top of this file).
    void idle(int device)
    {
        (void)hipSetDevice(device);
        for (Slot &s : slot)
            if (s.stream) (void)hipStreamSynchronize(s.stream);
    }
};

// A NULL check and the context's device made current.
#define BATCH_CTX(p, name)                             \
    if (!(p)) return fail(UTM_EINVAL, name " is NULL"); \
    HIP_TRY(hipSetDevice((p)->device))

// The device of a new context made current.
static int open_device(int device)
{
    int n = 0;
    HIP_TRY(hipGetDeviceCount(&n));
    if (device < 0 || device >= n) return fail(UTM_EINVAL, "device %d of %d", device, n);
    HIP_TRY(hipSetDevice(device));
    return UTM_OK;
}

// *ms += the time from event a to event b.
static int add_elapsed(double *ms, hipEvent_t a, hipEvent_t b)
{
    float t = 0;
    HIP_TRY(hipEventElapsedTime(&t, a, b));
    *ms += t;
    return UTM_OK;
}
