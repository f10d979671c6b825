// aix_owned.hpp — private to the library: the small owners behind the index handle (aix_handle.hpp) and the per-call resources of
// the files that work on it. Each frees what it holds in its destructor; all are move-only or fixed in place. The handle's byte ledger
// (device_bytes) is adjusted here and nowhere else: a slot that is bound to the ledger adds the COUNTED size of the block it takes and
// subtracts it when the block goes. Counted and allocated size are separate because they differ on purpose (a block of n ? n : 1
// entries counts n; the binned workspace is not part of the index and counts nothing).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <utility>

// A hipMalloc'd block that is never pooled and knows its size.
struct HBlock {
    void* p = nullptr;
    uint64_t bytes = 0, counted = 0;
    uint64_t* ledger = nullptr;                                  // belongs to the slot, not to the block: a move leaves both ledgers as they are bound
    HBlock() = default;
    explicit HBlock(uint64_t* l) : ledger(l) {}
    HBlock(const HBlock&) = delete;
    HBlock& operator=(const HBlock&) = delete;
    HBlock(HBlock&& o) noexcept { take(o); }
    HBlock& operator=(HBlock&& o) noexcept { if (this != &o) { drop(); take(o); } return *this; }
    ~HBlock() { drop(); }
    hipError_t alloc(uint64_t alloc_bytes, uint64_t counted_bytes) {
        drop();
        const hipError_t e = hipMalloc(&p, alloc_bytes);
        if (e != hipSuccess) { p = nullptr; return e; }
        hold(alloc_bytes, counted_bytes);
        return hipSuccess;
    }
    hipError_t alloc(uint64_t b) { return alloc(b, b); }
    void drop() { if (p) (void)hipFree(leak()); }
    void* leak() {                                               // gives the block up without freeing it
        void* q = p;
        if (ledger) *ledger -= counted;
        p = nullptr; bytes = counted = 0;
        return q;
    }
    template <class T> T* as() const { return (T*)p; }
    explicit operator bool() const { return p != nullptr; }

private:
    void hold(uint64_t b, uint64_t c) { bytes = b; counted = c; if (ledger) *ledger += c; }
    void take(HBlock& o) { const uint64_t b = o.bytes, c = o.counted; p = o.leak(); if (p) hold(b, c); }
};

// The grow-only form: ensure(need, counted, wait) keeps a block that is large enough; otherwise it runs wait() (whatever orders the call behind the
// users of the old block), drops the block and allocates `need`. Out of memory comes back as a value with the sticky error cleared and
// leaves the slot empty; what "does not fit" means to the call stays with the caller. `fits` (false = do not even ask the driver) is the
// caller's test hook.
struct GrowBlock : HBlock {
    using HBlock::HBlock;
    template <class Wait>
    hipError_t ensure(uint64_t need, uint64_t counted_bytes, Wait&& wait, bool fits = true) {
        if (need <= bytes) return hipSuccess;
        const hipError_t w = wait();
        if (w != hipSuccess) return w;
        drop();
        const hipError_t e = fits ? alloc(need, counted_bytes) : hipErrorOutOfMemory;
        if (e == hipErrorOutOfMemory) (void)hipGetLastError();
        return e;
    }
};

// A device pointer the handle either owns (copied at attach, freed at reset) or borrows from the caller. attach_owned, attach_borrowed
// and reset are the only ways its state changes.
struct Attached {
    void* p = nullptr;
    bool attached = false, owned = false;
    uint64_t counted = 0;
    uint64_t* ledger = nullptr;
    Attached() = default;
    explicit Attached(uint64_t* l) : ledger(l) {}
    Attached(const Attached&) = delete;
    Attached& operator=(const Attached&) = delete;
    ~Attached() { reset(); }
    void attach_owned(HBlock&& b) { reset(); const uint64_t c = b.counted; set(b.leak(), true, c); }
    void attach_borrowed(const void* q, uint64_t counted_bytes = 0) { reset(); set(const_cast<void*>(q), false, counted_bytes); }
    void reset() {
        if (owned && p) (void)hipFree(p);
        if (ledger) *ledger -= counted;
        p = nullptr; attached = owned = false; counted = 0;
    }
    template <class T> T* as() const { return (T*)p; }

private:
    void set(void* q, bool own, uint64_t c) { p = q; attached = true; owned = own; counted = c; if (ledger) *ledger += c; }
};

// Lazily created stream / event, destroyed in the destructor. wait_first: synchronise before destroying — for a stream whose work
// writes blocks that are released right behind it, and for an event that stands for the last user of such blocks.
struct Stream {
    hipStream_t s = nullptr;
    bool wait_first = false;
    Stream() = default;
    explicit Stream(bool wait) : wait_first(wait) {}
    Stream(const Stream&) = delete;
    Stream& operator=(const Stream&) = delete;
    Stream(Stream&& o) noexcept : s(o.s), wait_first(o.wait_first) { o.s = nullptr; }
    Stream& operator=(Stream&& o) noexcept { if (this != &o) { reset(); s = o.s; wait_first = o.wait_first; o.s = nullptr; } return *this; }
    ~Stream() { reset(); }
    hipError_t create() { return s ? hipSuccess : made(hipStreamCreateWithFlags(&s, hipStreamNonBlocking)); }
    hipError_t create_cu_mask(uint32_t words, const uint32_t* mask) { return s ? hipSuccess : made(hipExtStreamCreateWithCUMask(&s, words, mask)); }
    void reset() { if (s) { if (wait_first) (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); s = nullptr; } }
    operator hipStream_t() const { return s; }

private:
    hipError_t made(hipError_t e) { if (e != hipSuccess) s = nullptr; return e; }
};

struct Event {
    hipEvent_t e = nullptr;
    bool wait_first = false;
    Event() = default;
    explicit Event(bool wait) : wait_first(wait) {}
    Event(const Event&) = delete;
    Event& operator=(const Event&) = delete;
    Event(Event&& o) noexcept : e(o.e), wait_first(o.wait_first) { o.e = nullptr; }
    Event& operator=(Event&& o) noexcept { if (this != &o) { reset(); e = o.e; wait_first = o.wait_first; o.e = nullptr; } return *this; }
    ~Event() { reset(); }
    hipError_t create(unsigned flags = hipEventDisableTiming) {
        if (e) return hipSuccess;
        const hipError_t st = hipEventCreateWithFlags(&e, flags);
        if (st != hipSuccess) e = nullptr;
        return st;
    }
    void reset() { if (e) { if (wait_first) (void)hipEventSynchronize(e); (void)hipEventDestroy(e); e = nullptr; } }
    operator hipEvent_t() const { return e; }
};

// A pinned host block (hipHostMalloc), freed in the destructor.
struct PinnedBlock {
    void* p = nullptr;
    PinnedBlock() = default;
    PinnedBlock(const PinnedBlock&) = delete;
    PinnedBlock& operator=(const PinnedBlock&) = delete;
    ~PinnedBlock() { if (p) (void)hipHostFree(p); }
    hipError_t alloc(uint64_t bytes, unsigned flags) {       // keeps a block it already has
        if (p) return hipSuccess;
        const hipError_t e = hipHostMalloc(&p, bytes, flags);
        if (e != hipSuccess) p = nullptr;
        return e;
    }
};

// records `ev` on `s` when the frame is left, on every path: what was enqueued before a failure still uses the workspace the event guards
struct RecordOnExit {
    hipEvent_t ev; hipStream_t s;
    ~RecordOnExit() { (void)hipEventRecord(ev, s); }
};

// A call that fails in the middle leaves with work possibly queued on its side streams, which write blocks the next call reuses at
// once: unless disarmed, the guard waits for the given streams (null entries are skipped) before the call returns.
template <int N>
struct DrainOnError {
    const Stream* streams[N];                                    // read at exit: a side stream made during the call is drained too
    bool armed = true;
    ~DrainOnError() {
        if (armed) for (const Stream* st : streams) if (st->s) (void)hipStreamSynchronize(st->s);
    }
};
