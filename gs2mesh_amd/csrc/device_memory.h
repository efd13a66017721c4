// device_memory.h -- who owns the device memory of the native handles.  Host code only: included by raster_api.hip,
// tsdf_api.hip and png_encode.hip, and compiled as it is against the CPU emulator's platform.h by the tests.
//
//   DeviceBuffer   one hipMalloc allocation, grow-only
//   PinnedBuffer   one hipHostMalloc allocation
//   ScratchArena   one DeviceBuffer carved into the temporaries of a call
//   EventPool      the recycled event pairs of the stage timers
//   StageTimer     one timed stage launch: a rocTX range and, when timing is on, an event pair of the pool around it
//
// Two rules.  Growth frees with the SYNCHRONISING hipFree before it allocates, so nothing in flight can still be using the
// old memory and no call site has to think about it (contents are not kept).  And none of these types may be a static
// object: a destructor that runs at process exit would free device memory after the HIP runtime has shut down.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "api_check.h"
#include "platform.h"
#include "roctx_ranges.h"

template <typename T>
class DeviceBuffer {
    T* p_ = nullptr;
    size_t cap_ = 0;   // elements

    int regrow(size_t need, size_t n) {
        if (p_) {
            T* old = p_;
            p_ = nullptr;
            cap_ = 0;
            GS2M_HIPCHK(hipFree(old));  // synchronises: safe w.r.t. in-flight work
        }
        hipError_t e = n < need || n > SIZE_MAX / sizeof(T) ? hipErrorOutOfMemory : hipMalloc((void**)&p_, n * sizeof(T));
        if (e != hipSuccess) {
            p_ = nullptr;
            gs2m_set_error("hipMalloc of %zu x %zu bytes failed: %s", n, sizeof(T), hipGetErrorString(e));
            return 1;
        }
        cap_ = n;
        return 0;
    }

public:
    DeviceBuffer() = default;
    DeviceBuffer(const DeviceBuffer&) = delete;
    DeviceBuffer& operator=(const DeviceBuffer&) = delete;
    ~DeviceBuffer() { (void)hipFree(p_); }
    T* get() const { return p_; }
    size_t capacity() const { return cap_; }
    // Room for `need` elements, with headroom when it has to grow.  On failure (1, error set) the buffer is empty.
    int reserve(size_t need) { return p_ && need <= cap_ ? 0 : regrow(need, need + need / 8 + 64); }
    // The same without headroom: pools and tables whose size is fixed when their handle is created.
    int reserve_exact(size_t n) { return p_ && n <= cap_ ? 0 : regrow(n, n); }
};

template <typename T>
class PinnedBuffer {   // page-locked host memory of a fixed size
    T* p_ = nullptr;
    size_t cap_ = 0;

public:
    PinnedBuffer() = default;
    PinnedBuffer(const PinnedBuffer&) = delete;
    PinnedBuffer& operator=(const PinnedBuffer&) = delete;
    ~PinnedBuffer() { (void)hipHostFree(p_); }
    T* get() const { return p_; }
    size_t capacity() const { return cap_; }
    int reserve(size_t n) {
        if (p_ && n <= cap_) return 0;
        (void)hipHostFree(p_);
        p_ = nullptr;
        cap_ = 0;
        hipError_t e = n > SIZE_MAX / sizeof(T) ? hipErrorOutOfMemory : hipHostMalloc((void**)&p_, n * sizeof(T));
        if (e != hipSuccess) {
            p_ = nullptr;
            gs2m_set_error("hipHostMalloc of %zu x %zu bytes failed: %s", n, sizeof(T), hipGetErrorString(e));
            return 1;
        }
        cap_ = n;
        return 0;
    }
};

// Grow-only scratch of one call's temporaries: they are carved out of ONE allocation that survives the call (a hipMalloc /
// hipFree pair per temporary cost the mesh passes 69 ms for 0.9 ms of kernels).  A call names its sub-buffers once,
//     unsigned *a, *b;  if (arena.carve(arena_sub(a, n), arena_sub(b, m))) return 1;
// and the arena sizes itself from the same list it hands the pointers out from, each 256-byte aligned.
template <typename T>
struct ArenaSub {
    T*& out;
    size_t count;
};
template <typename T>
ArenaSub<T> arena_sub(T*& out, size_t count) {
    return ArenaSub<T>{out, count};
}

class ScratchArena {
    DeviceBuffer<char> buf_;
    static size_t pad(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

public:
    const char* base() const { return buf_.get(); }
    size_t capacity() const { return buf_.capacity(); }   // bytes
    template <typename... T>
    int carve(ArenaSub<T>... subs) {
        const size_t total = (size_t(0) + ... + pad(sizeof(T) * subs.count));
        if (buf_.reserve(total)) return 1;
        size_t off = 0;
        ((subs.out = reinterpret_cast<T*>(buf_.get() + off), off += pad(sizeof(T) * subs.count)), ...);
        return 0;
    }
};

// Event pairs around timed launches: recorded pairs wait in `live` until drain() reads them and recycles their events.
class EventPool {
    struct Pair {
        int stage;
        hipEvent_t a, b;
        int weight;
    };
    std::vector<Pair> live_;         // recorded, not yet read
    std::vector<hipEvent_t> free_;   // recycled events

public:
    EventPool() = default;
    EventPool(const EventPool&) = delete;
    EventPool& operator=(const EventPool&) = delete;
    ~EventPool() {
        for (auto& p : live_) {
            (void)hipEventDestroy(p.a);
            (void)hipEventDestroy(p.b);
        }
        for (auto e : free_) (void)hipEventDestroy(e);
    }
    hipEvent_t get() {   // null when no event can be created: the caller then leaves the launch untimed
        if (!free_.empty()) {
            hipEvent_t e = free_.back();
            free_.pop_back();
            return e;
        }
        hipEvent_t e;
        return hipEventCreate(&e) == hipSuccess ? e : nullptr;
    }
    void put(hipEvent_t e) {   // an event of get() that was never pushed goes back
        if (e) free_.push_back(e);
    }
    // a and b were recorded around a launch of `stage`; it counts as `weight` launches (a batch: its frames)
    void push(int stage, hipEvent_t a, hipEvent_t b, int weight = 1) { live_.push_back({stage, a, b, weight}); }
    // adds what was pushed since the last drain to total_ms[n_stages] / launches[n_stages]; the stream must be idle
    void drain(double* total_ms, int64_t* launches, int n_stages) {
        for (auto& p : live_) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess && p.stage >= 0 && p.stage < n_stages) {
                total_ms[p.stage] += ms;
                launches[p.stage] += p.weight;
            }
            free_.push_back(p.a);
            free_.push_back(p.b);
        }
        live_.clear();
    }
};

// RAII around one stage launch: a rocTX range `name` (GS2M_ROCTX=1) and, when `enabled`, an event pair recorded on `st` and
// pushed to the pool as `weight` launches of `stage`.  Without events to be had the launch goes untimed.
class StageTimer {
    EventPool& pool_;
    hipStream_t st_;
    hipEvent_t a_ = nullptr, b_ = nullptr;
    int stage_, weight_;
    Gs2mRange range_;

public:
    StageTimer(EventPool& pool, bool enabled, hipStream_t st, int stage, const char* name, int weight = 1)
        : pool_(pool), st_(st), stage_(stage), weight_(weight), range_(name) {
        if (enabled) {
            a_ = pool_.get();
            b_ = pool_.get();
            if (a_ && b_) {
                (void)hipEventRecord(a_, st_);
            } else {   // half a pair times nothing
                pool_.put(a_);
                pool_.put(b_);
                a_ = b_ = nullptr;
            }
        }
    }
    StageTimer(const StageTimer&) = delete;
    StageTimer& operator=(const StageTimer&) = delete;
    ~StageTimer() {
        if (a_) {
            (void)hipEventRecord(b_, st_);
            pool_.push(stage_, a_, b_, weight_);
        }
    }
};
