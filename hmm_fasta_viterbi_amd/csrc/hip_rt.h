// hip_rt.h -- the host device layer's HIP plumbing, shared by msv_device.cpp, vit_device.cpp,
// msv_multi.cpp and the host half of fasta_device.hip: the device guard, the status mapping and its
// return-on-error macro, move-only owners of device buffers, pinned buffers, streams and events, and the
// checks every host entry point opens with.
//
// The owners never switch devices and never synchronise on their own (the one exception is documented at
// DeviceBuffer::replace_with): whoever destroys or shrinks one does so with its device current and with
// nothing in flight that uses it.  No virtuals, no heap allocation.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <utility>

#include "msv.h"
#include "msv_plan.h"

namespace msvrt {

// Every launch addresses < 2^32 residue bytes and fewer than kMaxLaunchSeqs sequences (msv_plan.h).
using msvplan::kChunkBytes;
using msvplan::kMaxLaunchSeqs;

struct DeviceGuard {
    int prev = -1;
    bool ok = false;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        ok = hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
};

inline msv_status hip_status(hipError_t e) {
    if (e == hipSuccess) return MSV_OK;
    if (e == hipErrorOutOfMemory) return MSV_ERR_OUT_OF_MEMORY;
    if (e == hipErrorNoDevice || e == hipErrorInvalidDevice) return MSV_ERR_NO_DEVICE;
    return MSV_ERR_HIP;
}

#define MSV_HIP(call)                                       \
    do {                                                    \
        hipError_t e_ = (call);                             \
        if (e_ != hipSuccess) return msvrt::hip_status(e_); \
    } while (0)

// The persistent grid that fills `device` with `kernel` at `threads` per block: the blocks one CU holds times
// the CUs.  When only the occupancy query fails, *blocks is one block per CU (0 when the CU count is unknown).
inline hipError_t resident_blocks(int device, const void* kernel, int threads, int* blocks) {
    int cus = 0, per_cu = 0;
    *blocks = 0;
    hipError_t e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device);
    if (e != hipSuccess) return e;
    e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, threads, 0);
    *blocks = cus * (e == hipSuccess ? std::max(1, per_cu) : 1);
    return e;
}

// Validates a CSR (offsets non-decreasing) and finds its longest sequence and its residue count.
inline msv_status csr_extent(const uint64_t* offsets, uint64_t n, uint64_t* maxL, uint64_t* total) {
    uint64_t longest = 0;
    for (uint64_t s = 0; s < n; ++s) {
        if (offsets[s + 1] < offsets[s]) return MSV_ERR_INVALID_ARGUMENT;
        longest = std::max<uint64_t>(longest, offsets[s + 1] - offsets[s]);
    }
    *maxL = longest;
    *total = n ? offsets[n] - offsets[0] : 0;
    return MSV_OK;
}

// Owner of one hipMalloc allocation of `capacity()` elements.  Converts to the raw pointer.
template <typename T>
class DeviceBuffer {
public:
    DeviceBuffer() = default;
    DeviceBuffer(DeviceBuffer&& o) noexcept : p_(std::exchange(o.p_, nullptr)), cap_(std::exchange(o.cap_, 0)) {}
    DeviceBuffer& operator=(DeviceBuffer&& o) noexcept {
        if (this != &o) {
            reset();
            p_ = std::exchange(o.p_, nullptr);
            cap_ = std::exchange(o.cap_, 0);
        }
        return *this;
    }
    ~DeviceBuffer() { reset(); }

    T* get() const { return p_; }
    operator T*() const { return p_; }
    size_t capacity() const { return cap_; }
    void reset() {
        if (p_) (void)hipFree(p_);
        p_ = nullptr;
        cap_ = 0;
    }
    // Room for n elements: nothing when they fit, else the allocation is freed and one of max(n, 1) made
    // (contents are not kept, no growth factor).
    hipError_t reserve(size_t n) {
        if (p_ && n <= cap_) return hipSuccess;
        reset();
        n = std::max<size_t>(n, 1);
        const hipError_t e = hipMalloc(reinterpret_cast<void**>(&p_), n * sizeof(T));
        if (e == hipSuccess) cap_ = n;
        else p_ = nullptr;
        return e;
    }
    // Uploads host[0 .. n) into a NEW allocation and adopts it; on failure the old one is untouched.  The
    // old allocation may still be read by a launch in flight on any stream, so, when there is one, the
    // device is synchronised before it is freed (the holders' only synchronisation).
    hipError_t replace_with(const T* host, size_t n) {
        DeviceBuffer fresh;
        hipError_t e = fresh.reserve(n);
        if (e == hipSuccess) e = hipMemcpy(fresh.p_, host, n * sizeof(T), hipMemcpyHostToDevice);
        if (e != hipSuccess) return e;
        if (p_) (void)hipDeviceSynchronize();
        *this = std::move(fresh);
        return hipSuccess;
    }

private:
    T* p_ = nullptr;
    size_t cap_ = 0;
};

// The same for page-locked host memory (hipHostMalloc with the caller's flags).
template <typename T>
class PinnedBuffer {
public:
    PinnedBuffer() = default;
    PinnedBuffer(PinnedBuffer&& o) noexcept : p_(std::exchange(o.p_, nullptr)), cap_(std::exchange(o.cap_, 0)) {}
    PinnedBuffer& operator=(PinnedBuffer&& o) noexcept {
        if (this != &o) {
            reset();
            p_ = std::exchange(o.p_, nullptr);
            cap_ = std::exchange(o.cap_, 0);
        }
        return *this;
    }
    ~PinnedBuffer() { reset(); }

    T* get() const { return p_; }
    operator T*() const { return p_; }
    size_t capacity() const { return cap_; }
    void reset() {
        if (p_) (void)hipHostFree(p_);
        p_ = nullptr;
        cap_ = 0;
    }
    hipError_t reserve(size_t n, unsigned flags) {
        if (p_ && n <= cap_) return hipSuccess;
        reset();
        n = std::max<size_t>(n, 1);
        const hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&p_), n * sizeof(T), flags);
        if (e == hipSuccess) cap_ = n;
        else p_ = nullptr;
        return e;
    }

private:
    T* p_ = nullptr;
    size_t cap_ = 0;
};

// Owners of a stream and of an event, created on demand (create is a no-op once created).  Both convert
// to the raw handle.
class Stream {
public:
    Stream() = default;
    Stream(Stream&& o) noexcept : s_(std::exchange(o.s_, nullptr)) {}
    Stream& operator=(Stream&& o) noexcept {
        if (this != &o) {
            reset();
            s_ = std::exchange(o.s_, nullptr);
        }
        return *this;
    }
    ~Stream() { reset(); }
    hipError_t create(unsigned flags) { return s_ ? hipSuccess : hipStreamCreateWithFlags(&s_, flags); }
    operator hipStream_t() const { return s_; }
    void reset() {
        if (s_) (void)hipStreamDestroy(s_);
        s_ = nullptr;
    }

private:
    hipStream_t s_ = nullptr;
};

class Event {
public:
    Event() = default;
    Event(Event&& o) noexcept : e_(std::exchange(o.e_, nullptr)) {}
    Event& operator=(Event&& o) noexcept {
        if (this != &o) {
            reset();
            e_ = std::exchange(o.e_, nullptr);
        }
        return *this;
    }
    ~Event() { reset(); }
    hipError_t create(unsigned flags) { return e_ ? hipSuccess : hipEventCreateWithFlags(&e_, flags); }
    operator hipEvent_t() const { return e_; }
    void reset() {
        if (e_) (void)hipEventDestroy(e_);
        e_ = nullptr;
    }

private:
    hipEvent_t e_ = nullptr;
};

// Synchronises up to three streams when a host call returns early: copies that read its pinned staging
// (rewritten by the next call) and kernels that write its buffers may still be queued.  disarm() on the
// path that has synchronised itself.
class StreamDrain {
public:
    explicit StreamDrain(hipStream_t a, hipStream_t b = nullptr, hipStream_t c = nullptr) : s_{a, b, c} {}
    StreamDrain(const StreamDrain&) = delete;
    StreamDrain& operator=(const StreamDrain&) = delete;
    ~StreamDrain() {
        if (armed_)
            for (hipStream_t x : s_)
                if (x) (void)hipStreamSynchronize(x);
    }
    void disarm() { armed_ = false; }

private:
    hipStream_t s_[3];
    bool armed_ = true;
};

// Device address of page-locked host memory that kernels can read or write directly (nullptr for pageable
// memory).  Host paths then need no score D2H: the kernels' stores cross PCIe as they are made (a few MB of
// posted writes spread over the launch), and the end-of-kernel system-scope release makes them visible
// before the completion the host waits on.  (A staged D2H of the scores was dispatched as a blit KERNEL
// when queued behind the next call's launch, and starved there: the persistent MSV grid holds every CU --
// profiles/r02_host_pipeline_timeline.txt.)  The same alias lets a kernel READ page-locked residues in
// place: see msv_score_batch.
template <typename T>
T* mapped_host(T* host) {
    hipPointerAttribute_t at{};
    void* h = const_cast<void*>(static_cast<const void*>(host));
    if (hipPointerGetAttributes(&at, h) != hipSuccess) {
        (void)hipGetLastError();  // pageable memory is not an error here
        return nullptr;
    }
    if (at.type != hipMemoryTypeHost) return nullptr;
    void* d = nullptr;
    if (hipHostGetDevicePointer(&d, h, 0) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    return static_cast<T*>(d);
}

}  // namespace msvrt
