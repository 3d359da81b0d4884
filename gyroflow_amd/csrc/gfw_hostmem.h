// gfw_hostmem.h — host only: the owning types of a context's device memory, pinned memory and events, and the staging ring made of them.
// None of them calls into HIP for a handle that was never created: a context that never met a device (gfw_debug_jit_key*) is destroyed without one.
#pragma once
#include <hip/hip_runtime.h>
#include <assert.h>
#include <stddef.h>
#include "gfw_layout.h"

// Device (hipMalloc) or pinned host (hipHostMalloc) memory that grows on demand; growth does not preserve contents.  Move-only.
template <bool PINNED>
struct OwnedBuf {
    void *ptr = nullptr; size_t cap = 0;
    OwnedBuf() = default;
    OwnedBuf(OwnedBuf &&o) noexcept : ptr(o.ptr), cap(o.cap) { o.ptr = nullptr; o.cap = 0; }
    OwnedBuf &operator=(OwnedBuf &&o) noexcept { if (this != &o) { release(); ptr = o.ptr; cap = o.cap; o.ptr = nullptr; o.cap = 0; } return *this; }
    ~OwnedBuf() { release(); }
    hipError_t ensure(size_t n) {
        if (n <= cap) return hipSuccess;
        release();
        const hipError_t e = PINNED ? hipHostMalloc(&ptr, n, hipHostMallocDefault) : hipMalloc(&ptr, n);
        if (e == hipSuccess) cap = n; else ptr = nullptr;
        return e;
    }
    void release() { if (ptr) (void)(PINNED ? hipHostFree(ptr) : hipFree(ptr)); ptr = nullptr; cap = 0; }
};
typedef OwnedBuf<false> DevBuf;
typedef OwnedBuf<true> PinnedBuf;

// An event, created at its first record().  Waiting for one that was never recorded is a no-op.  Move-only.
struct Event {
    hipEvent_t ev = nullptr; unsigned flags;
    explicit Event(unsigned f = hipEventDisableTiming) : flags(f) {}      // (hipEventDefault: the profiling brackets, which are timed)
    Event(Event &&o) noexcept : ev(o.ev), flags(o.flags) { o.ev = nullptr; }
    Event &operator=(Event &&o) noexcept { if (this != &o) { if (ev) (void)hipEventDestroy(ev); ev = o.ev; flags = o.flags; o.ev = nullptr; } return *this; }
    ~Event() { if (ev) (void)hipEventDestroy(ev); }
    bool recorded() const { return ev != nullptr; }
    hipError_t record(hipStream_t s) {
        if (!ev) { const hipError_t e = hipEventCreateWithFlags(&ev, flags); if (e != hipSuccess) { ev = nullptr; return e; } }
        return hipEventRecord(ev, s);
    }
    hipError_t wait_host() const { return ev ? hipEventSynchronize(ev) : hipSuccess; }
    hipError_t wait_on(hipStream_t s) const { return ev ? hipStreamWaitEvent(s, ev, 0) : hipSuccess; }
};

// What the host writes for a kernel to read: filled in pinned memory, copied to the device side by the slot's user.  A slot is free when the event recorded behind
// its last enqueued reader has completed: the user calls free_again.record(stream) after the last thing it enqueues that reads the slot.
struct StagingSlot { PinnedBuf h; DevBuf d; Event free_again; };
template <int N>
struct StagingRing {
    StagingSlot slots[N]; int next = 0;
    hipError_t reserve(size_t bytes) {               // every slot at once (where a failure has to show, or the first use is to pay for all)
        hipError_t e = hipSuccess;
        for (int i = 0; i < N && e == hipSuccess; ++i) { e = slots[i].h.ensure(bytes); if (e == hipSuccess) e = slots[i].d.ensure(bytes); }
        return e;
    }
    // The next slot: the host waits until it is free, then both sides get room for `bytes`.  `reader`: the stream the slot is used on — a user that records
    // free_again ahead of its kernel leaves a reader of the device side in flight there, so that stream is drained before the device side is replaced.
    hipError_t acquire(size_t bytes, hipStream_t reader, StagingSlot **out) {
        StagingSlot &s = slots[next];
        next = (next + 1) % N;
        hipError_t e = s.free_again.wait_host();
        if (e == hipSuccess && s.d.ptr && s.d.cap < bytes) e = hipStreamSynchronize(reader);
        if (e == hipSuccess) e = s.h.ensure(bytes);
        if (e == hipSuccess) e = s.d.ensure(bytes);
        *out = &s;
        return e;
    }
};

// An acquired slot as the block a call stages (BlockLayout, gfw_layout.h): the packers fill it at (h, d), one copy takes `total` bytes up.  Where free_again is
// recorded is the call's own decision (behind the copy, or behind the last kernel that reads the device side): see StagingRing::acquire.
struct StagedBlock {
    StagingSlot *slot = nullptr;
    char *h() const { return (char *)slot->h.ptr; }
    const char *d() const { return (const char *)slot->d.ptr; }
    hipError_t upload(size_t total, hipStream_t s) const { return hipMemcpyAsync(slot->d.ptr, slot->h.ptr, total, hipMemcpyHostToDevice, s); }
    hipError_t free_again(hipStream_t s) const { return slot->free_again.record(s); }
};

// The outputs of one call.  add() every output (a NULL one stays NULL), reserve(), then dev(i) is what the kernels write: the caller's pointer when the outputs are
// device memory, otherwise a slice of `buf`, which finish() copies to the caller's host memory.  ONE buffer serves every entry point of a context: a call with host
// outputs synchronises before it returns, so no earlier call's results are still in the buffer when the next one takes it (or lets it grow, which frees it).
struct CallOutputs {
    struct Part { void *caller; size_t at, bytes; };
    DevBuf &buf; const bool on_device;
    static constexpr int kMaxParts = 6;              // the most any call adds: optical flow (next, status, iterations, grid points, grid counts, pair firsts)
    Part parts[kMaxParts]; int n = 0; BlockLayout layout;
    CallOutputs(DevBuf &b, int out_on_device) : buf(b), on_device(out_on_device != 0) {}
    int add(void *caller, size_t bytes) { assert(n < kMaxParts); parts[n] = Part{caller, caller ? layout.add(bytes) : 0, bytes}; return n++; }
    hipError_t reserve() { return on_device ? hipSuccess : buf.ensure(layout.total); }
    void *dev(int i) const { return !parts[i].caller || on_device ? parts[i].caller : (char *)buf.ptr + parts[i].at; }
    // the copies back, then the one rule of when a call waits: a synchronous context, or results the caller reads from host memory on return
    hipError_t finish(hipStream_t s, bool synchronous) const {
        hipError_t e = hipSuccess;
        for (int i = 0; i < n && !on_device && e == hipSuccess; ++i)
            if (parts[i].caller && parts[i].bytes) e = hipMemcpyAsync(parts[i].caller, dev(i), parts[i].bytes, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess && (synchronous || !on_device)) e = hipStreamSynchronize(s);
        return e;
    }
};
