// hip_rt.h -- the host device layer's HIP plumbing, shared by msv_device.cpp, msv_multi.cpp, the host half of
// fasta_device.hip and, through stage_profile.h, the Viterbi and Forward layers: the device guard, the status
// mapping and its return-on-error macro, move-only owners of device buffers, pinned buffers, streams and events,
// the checks every host entry point opens with, the staging of one host batch (CsrStaging), and the few lines every
// device layer would otherwise spell for itself: a kernel's full grid and footprint, the time between two events, a
// host list's upload, the NaN pre-fill of scores.
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
#include <vector>

#include "item_plan.h"
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

// resident_blocks for the answers that need a grid whatever the queries say: at least one block.
inline uint32_t full_grid(int device, const void* kernel, int threads) {
    int blocks = 0;
    (void)resident_blocks(device, kernel, threads, &blocks);
    return static_cast<uint32_t>(std::max(1, blocks));
}

// What a kernel keeps per thread in scratch and per block in LDS, and its vector registers (left as they are when
// the query fails).
inline void kernel_footprint(const void* kernel, uint32_t* scratch, uint32_t* lds, uint32_t* vgprs = nullptr) {
    hipFuncAttributes fa{};
    if (hipFuncGetAttributes(&fa, kernel) != hipSuccess) return;
    if (scratch) *scratch = static_cast<uint32_t>(fa.localSizeBytes);
    if (lds) *lds = static_cast<uint32_t>(fa.sharedSizeBytes);
    if (vgprs) *vgprs = static_cast<uint32_t>(fa.numRegs);
}

// Validates a CSR (offsets non-decreasing) and finds its longest sequence and its residue count (item_plan.h).
using itemplan::csr_extent;

// Owner of one allocation of `capacity()` elements: device memory (hipMalloc) or, Pinned, page-locked host
// memory (hipHostMalloc with the caller's flags).  Converts to the raw pointer.
template <typename T, bool Pinned>
class Buffer {
public:
    Buffer() = default;
    Buffer(Buffer&& o) noexcept : p_(std::exchange(o.p_, nullptr)), cap_(std::exchange(o.cap_, 0)) {}
    Buffer& operator=(Buffer&& o) noexcept {
        if (this != &o) {
            reset();
            p_ = std::exchange(o.p_, nullptr);
            cap_ = std::exchange(o.cap_, 0);
        }
        return *this;
    }
    ~Buffer() { reset(); }

    T* get() const { return p_; }
    operator T*() const { return p_; }
    size_t capacity() const { return cap_; }
    void reset() {
        if (p_) (void)(Pinned ? hipHostFree(p_) : hipFree(p_));
        p_ = nullptr;
        cap_ = 0;
    }
    // Room for n elements: nothing when they fit, else the allocation is freed and one of max(n, 1) made
    // (contents are not kept, no growth factor).
    hipError_t reserve(size_t n, unsigned pinned_flags = hipHostMallocDefault) {
        if (p_ && n <= cap_) return hipSuccess;
        reset();
        n = std::max<size_t>(n, 1);
        void** const out = reinterpret_cast<void**>(&p_);
        const hipError_t e = Pinned ? hipHostMalloc(out, n * sizeof(T), pinned_flags) : hipMalloc(out, n * sizeof(T));
        if (e == hipSuccess) cap_ = n;
        else p_ = nullptr;
        return e;
    }
    // Device buffers: uploads host[0 .. n) into a NEW allocation and adopts it; on failure the old one is
    // untouched.  The old allocation may still be read by a launch in flight on any stream, so, when there is
    // one, the device is synchronised before it is freed (the holders' only synchronisation).
    hipError_t replace_with(const T* host, size_t n) {
        static_assert(!Pinned, "replace_with uploads to the device");
        Buffer fresh;
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
template <typename T>
using DeviceBuffer = Buffer<T, false>;
template <typename T>
using PinnedBuffer = Buffer<T, true>;

// Owners of a stream and of an event, created on demand (create is a no-op once created).  Both convert
// to the raw handle.
template <typename H, hipError_t (*Create)(H*, unsigned), hipError_t (*Destroy)(H)>
class Handle {
public:
    Handle() = default;
    Handle(Handle&& o) noexcept : h_(std::exchange(o.h_, nullptr)) {}
    Handle& operator=(Handle&& o) noexcept {
        if (this != &o) {
            reset();
            h_ = std::exchange(o.h_, nullptr);
        }
        return *this;
    }
    ~Handle() { reset(); }
    hipError_t create(unsigned flags) { return h_ ? hipSuccess : Create(&h_, flags); }
    operator H() const { return h_; }
    void reset() {
        if (h_) (void)Destroy(h_);
        h_ = nullptr;
    }

private:
    H h_ = nullptr;
};
using Stream = Handle<hipStream_t, hipStreamCreateWithFlags, hipStreamDestroy>;
using Event = Handle<hipEvent_t, hipEventCreateWithFlags, hipEventDestroy>;

// Milliseconds between two recorded, completed events (0 when the runtime cannot say).
inline float elapsed(hipEvent_t a, hipEvent_t b) {
    float ms = 0.0f;
    return hipEventElapsedTime(&ms, a, b) == hipSuccess ? ms : 0.0f;
}

// Room for a host list on the device and its copy queued on `st` (the list outlives the copy: the caller's).
template <class T>
hipError_t upload(DeviceBuffer<T>& d, const std::vector<T>& h, hipStream_t st) {
    hipError_t e = d.reserve(h.size());
    if (e == hipSuccess && !h.empty())
        e = hipMemcpyAsync(d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, st);
    return e;
}

// n scores of quiet-NaN bits: what an entry that the kernels refuse keeps.
inline hipError_t fill_nan(float* d, size_t n, hipStream_t st) {
    return hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(d), 0x7fc00000, n, st);
}

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

// One staged host batch: the device residues, offsets, dequeue order and scores, and the pinned host copy of
// the rebased offsets (a true async DMA; rewritten by the next upload, so whoever uploads lets the stream
// finish first: a StreamDrain on early returns).  Never switches devices, never synchronises.
struct CsrStaging {
    DeviceBuffer<uint8_t> d_res;
    DeviceBuffer<uint64_t> d_off;
    DeviceBuffer<uint32_t> d_order;
    DeviceBuffer<float> d_scores;
    PinnedBuffer<uint64_t> h_off;

    // Room for `words` offset words (device and h_off) and `bytes` residue bytes.  THE rule for batches without
    // residues: d_res always holds a readable byte (reserve never allocates less), since for an empty sequence
    // a kernel computes one discarded row on byte 0.  readable(): the residues a launch over `bytes` reads.
    hipError_t reserve_inputs(uint64_t words, uint64_t bytes) {
        hipError_t e = d_res.reserve(bytes);
        if (e == hipSuccess) e = d_off.reserve(words);
        return e == hipSuccess ? h_off.reserve(words) : e;
    }
    const uint8_t* readable(const uint8_t* src, uint64_t bytes) const { return bytes ? src : d_res.get(); }
    // Room for the dequeue order of n sequences and for `scores` scores (0: they are written elsewhere).
    hipError_t reserve_results(uint64_t n, uint64_t scores) {
        const hipError_t e = d_order.reserve(n);
        return e == hipSuccess && scores ? d_scores.reserve(scores) : e;
    }
    // Stages sequences [first, last) of a host CSR as one batch (none: `offsets` may be null): reserves the
    // inputs, rebases the offsets into h_off, queues their H2D on `off_stream` and, if copy_residues (they
    // are not read in place) and there are any, the residues' on `res_stream`.  On one stream the residues go
    // first (msv_score_grid's 24 x 3 grid of pageable residues: 0.44 ms, against 0.46 ms behind the offsets'
    // copy); on two the offsets, which the order kernel waits for.
    hipError_t upload(const uint8_t* residues, const uint64_t* offsets, uint64_t first, uint64_t last,
                      bool copy_residues, hipStream_t off_stream, hipStream_t res_stream) {
        const uint64_t n = last - first, bytes = n && copy_residues ? offsets[last] - offsets[first] : 0;
        hipError_t e = reserve_inputs(n + 1, bytes);
        if (e != hipSuccess) return e;
        if (n) msvplan::rebase_offsets(offsets, first, last, h_off);
        else h_off[0] = 0;
        const auto copy_res = [&] {
            return bytes ? hipMemcpyAsync(d_res, residues + offsets[first], bytes, hipMemcpyHostToDevice, res_stream)
                         : hipSuccess;
        };
        if (off_stream == res_stream && (e = copy_res()) != hipSuccess) return e;
        e = hipMemcpyAsync(d_off, h_off, (n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, off_stream);
        return e == hipSuccess && off_stream != res_stream ? copy_res() : e;
    }
};

}  // namespace msvrt
