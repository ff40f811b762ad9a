// Owners of the library's HIP resources on the host side: device buffers, events and streams.
// Each frees what it holds when its owner goes; they are moved, never copied.  Their methods
// return hipError_t, so every translation unit reports a failure through its own error channel
// (ehm_err.h) with EHM_HIP_TRY.  After them the small helpers every host path repeats: the grid of
// a launch, a wall clock and the sizes behind the ehm_*_abi_sizes getters.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstddef>
#include <cstdint>
#include <utility>

#include "ehm_err.h"

// `expr` (a hipError_t) or return EHM_E_HIP with its text in `channel` (an ehm_err_channel)
#define EHM_HIP_TRY(channel, expr)                                                         \
    do {                                                                                   \
        const hipError_t e_ = (expr);                                                      \
        if (e_ != hipSuccess)                                                              \
            return (channel).fail(EHM_E_HIP, "%s failed: %s", #expr,                       \
                                  hipGetErrorString(e_));                                  \
    } while (0)

// workgroups of `block` threads that cover n items
inline unsigned blocks_of(long long n, int block) { return (unsigned)((n + block - 1) / block); }

inline double wall_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

// what every ehm_*_abi_sizes returns: the first min(n, known) of `all` into `sizes` (nullptr:
// none), and `known`
inline int ehm_copy_abi_sizes(const int64_t* all, int32_t known, int64_t* sizes, int32_t n) {
    for (int32_t k = 0; sizes && k < n && k < known; ++k) sizes[k] = all[k];
    return known;
}

// One device allocation of `cap` bytes (nullptr / 0: none).
struct DevBuf {
    void* ptr = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept { *this = std::move(o); }
    DevBuf& operator=(DevBuf&& o) noexcept {
        std::swap(ptr, o.ptr);
        std::swap(cap, o.cap);
        return *this;
    }
    ~DevBuf() { reset(); }
    explicit operator bool() const { return ptr != nullptr; }
    template <class T> T* as() const { return static_cast<T*>(ptr); }
    void reset() {
        if (ptr) (void)hipFree(ptr);
        ptr = nullptr;
        cap = 0;
    }
    // a new buffer of `bytes` (at least 1) in place of the held one
    hipError_t alloc(size_t bytes) {
        reset();
        const size_t want = bytes ? bytes : 1;
        const hipError_t e = hipMalloc(&ptr, want);
        if (e != hipSuccess) ptr = nullptr;
        else cap = want;
        return e;
    }
    // grow-only: at least `bytes` (and 4096); the contents are dropped when it grows
    hipError_t ensure(size_t bytes) {
        return bytes <= cap ? hipSuccess : alloc(std::max(bytes, (size_t)4096));
    }
    // a new buffer holding a copy of `bytes` of host memory
    hipError_t upload(const void* src, size_t bytes) {
        const hipError_t e = alloc(bytes);
        return (e != hipSuccess || !bytes) ? e : hipMemcpy(ptr, src, bytes, hipMemcpyHostToDevice);
    }
};

// One event (nullptr until created); converts to hipEvent_t.
struct Event {
    hipEvent_t ev = nullptr;
    Event() = default;
    Event(const Event&) = delete;
    Event& operator=(const Event&) = delete;
    Event(Event&& o) noexcept : ev(o.ev) { o.ev = nullptr; }
    Event& operator=(Event&& o) noexcept {
        std::swap(ev, o.ev);
        return *this;
    }
    ~Event() { reset(); }
    operator hipEvent_t() const { return ev; }
    void reset() {
        if (ev) (void)hipEventDestroy(ev);
        ev = nullptr;
    }
    hipError_t create() {
        reset();
        const hipError_t e = hipEventCreate(&ev);
        if (e != hipSuccess) ev = nullptr;
        return e;
    }
    // a new event, recorded on `s` (the time stamps of a run)
    static Event recorded(hipStream_t s) {
        Event v;
        if (v.create() == hipSuccess) (void)hipEventRecord(v.ev, s);
        return v;
    }
};

// The two events that time a launch.
struct EventPair {
    Event e0, e1;
    EventPair() {
        (void)e0.create();
        (void)e1.create();
    }
    void seconds(double* out) const {
        if (!out) return;
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, e0, e1);
        *out = ms * 1e-3;
    }
};

// One stream (nullptr until created); converts to hipStream_t.
struct Stream {
    hipStream_t s = nullptr;
    Stream() = default;
    Stream(const Stream&) = delete;
    Stream& operator=(const Stream&) = delete;
    ~Stream() {
        if (s) (void)hipStreamDestroy(s);
    }
    operator hipStream_t() const { return s; }
    hipError_t create() {
        const hipError_t e = hipStreamCreate(&s);
        if (e != hipSuccess) s = nullptr;
        return e;
    }
};
