// Who owns what on the host side: the one place of the library that allocates and frees device memory, pinned memory, events,
// streams and instantiated graphs.  Host code only.  Every owner is move-only, empty when default-constructed, and lets go in its
// destructor.
//
// An owner NEVER waits for the device.  Whoever replaces or destroys something that a running kernel or a replaying graph may
// still read waits first, at the call site (hipDeviceSynchronize / replay_quiesce).
//
// The first half (DevBuf, Owned) needs no HIP runtime.  Device memory goes through the two raw functions below: hierdiff_hip.hip
// defines them over hipMalloc / hipFree with the counters behind hd_live_allocations, and a stand-alone test defines them over
// malloc / free (tests/mem_owner_main.cpp).  The second half (pinned memory, events, streams, graphs) is compiled by hipcc only,
// inside hierdiff_hip.hip's translation unit (it uses its HIP_TRY / HD_TRY).
#pragma once

#include "../../include/hierdiff_hip.h"

#include <cstddef>
#include <utility>
#include <vector>

// HD_OK with *p set, or HD_E_NOMEM with *p null and the error text "hipMalloc: <reason>" in place (hd_last_error).
int hd_raw_alloc(void** p, size_t bytes);
// p came from hd_raw_alloc with this many bytes.
void hd_raw_free(void* p, size_t bytes);

// `count` elements of device memory (a count of 0 holds one element).  Converts to T*, so code that fills kernel arguments reads the
// member as it would a pointer.
template <typename T>
class DevBuf {
    T* p_ = nullptr;
    size_t cap_ = 0;                            // elements

public:
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) {
            release();
            p_ = o.p_; cap_ = o.cap_;
            o.p_ = nullptr; o.cap_ = 0;
        }
        return *this;
    }
    ~DevBuf() { release(); }

    operator T*() const { return p_; }
    size_t capacity() const { return cap_; }
    size_t bytes() const { return cap_ * sizeof(T); }

    void release() {
        if (p_) hd_raw_free(p_, bytes());
        p_ = nullptr; cap_ = 0;
    }
    // what it held goes first; a failure leaves it empty
    int alloc(size_t count) {
        release();
        if (count == 0) count = 1;
        void* q = nullptr;
        const int r = hd_raw_alloc(&q, count * sizeof(T));
        if (r != HD_OK) return r;
        p_ = static_cast<T*>(q); cap_ = count;
        return HD_OK;
    }
    int alloc_once(size_t count) { return p_ ? HD_OK : alloc(count); }
    // same address while `count` fits; otherwise a new block (the old one freed) and *moved set
    int grow(size_t count, bool* moved) {
        if (p_ && count <= cap_) return HD_OK;
        *moved = true;
        return alloc(count);
    }
};

// A handle that one call destroys: an event, a stream, an instantiated graph.
template <typename H, auto Destroy>
class Owned {
    H h_ = nullptr;

public:
    Owned() = default;
    Owned(Owned&& o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    Owned& operator=(Owned&& o) noexcept {
        if (this != &o) { reset(); h_ = o.h_; o.h_ = nullptr; }
        return *this;
    }
    ~Owned() { reset(); }

    operator H() const { return h_; }
    void reset() {
        if (h_) (void)Destroy(h_);
        h_ = nullptr;
    }
    void adopt(H h) { reset(); h_ = h; }        // a handle somebody just created
};

#ifdef __HIPCC__

#include <hip/hip_runtime.h>

using Event = Owned<hipEvent_t, hipEventDestroy>;
using Stream = Owned<hipStream_t, hipStreamDestroy>;
using GraphExec = Owned<hipGraphExec_t, hipGraphExecDestroy>;      // adopts what hipGraphInstantiate made
using PinnedBuf = Owned<char*, hipHostFree>;                       // pinned, device-visible host memory (mapped by default)

// `make(&handle, args...)` into an owner; a failed call leaves the owner as it was
template <typename H, auto D, typename Make, typename... A>
static hipError_t own(Owned<H, D>& o, Make make, A... args) {
    H h = nullptr;
    const hipError_t r = make(&h, args...);
    if (r == hipSuccess) o.adopt(h);
    return r;
}
static inline hipError_t event_create(Event& e, unsigned flags) { return own(e, hipEventCreateWithFlags, flags); }
static inline hipError_t stream_create(Stream& s, unsigned flags) { return own(s, hipStreamCreateWithFlags, flags); }
static inline hipError_t pinned_alloc(PinnedBuf& p, size_t bytes) {
    return own(p, [](char** q, size_t n) { return hipHostMalloc(reinterpret_cast<void**>(q), n, hipHostMallocDefault); }, bytes);
}

// `v` on the device (blocking copy from pageable memory)
template <typename T>
static int dev_upload(DevBuf<T>& b, const std::vector<T>& v) {
    HD_TRY(b.alloc(v.size()));
    if (!v.empty()) HIP_TRY(hipMemcpy(b, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return HD_OK;
}

#endif  // __HIPCC__
