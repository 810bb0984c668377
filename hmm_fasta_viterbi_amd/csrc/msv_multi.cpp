// msv_multi.cpp -- one batch over several GPUs from ONE process, with the score gather done by RCCL
// over xGMI (ncclCommInitAll, rccl.h:236; grouped ncclSend / ncclRecv, rccl.h:700-725).
//
// The reference has no multi-device path.  Sequences are independent, so the batch is cut
// into contiguous shards of ~equal residue count (msv_shard_bounds); one host thread per device
// uploads its shard (or, for page-locked residues, lets its kernel read them in place) and enqueues the
// longest-first order and ONE kernel launch on the device's stream;
// then a single RCCL group moves every shard's float scores into device 0's result buffer at the
// shard's offset (exact counts, no padding; rank 0's own shard goes through a self send/recv, so the
// exchange code runs even with one device), and one D2H returns them.  Only public msv.h entry points
// are used on the profiles; the context owns its streams, staging buffers and communicators.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <atomic>
#include <new>
#include <thread>
#include <vector>

#include "hip_rt.h"
#include "msv.h"

using msvrt::DeviceBuffer;
using msvrt::DeviceGuard;

// msv_device.cpp (library-internal): msv_score_batch_device for page-locked host residues (zero-copy twin).
extern "C" msv_status msv_score_batch_host_residues(msv_profile* p, const uint8_t* d_residues, uint64_t residues_len,
                                         const uint64_t* d_offsets, uint64_t n, const uint32_t* d_order,
                                         float* d_scores, void* stream);

namespace {

#define MM_NCCL(call)                                 \
    do {                                              \
        if ((call) != ncclSuccess) return MSV_ERR_RCCL; \
    } while (0)

struct Rank {
    msv_profile* profile = nullptr;
    int device = -1;
    uint32_t states = 0;  // of the profile's model
    // (declared before the buffers: a rank's members go in reverse order, the stream last, with the rank's
    // device current -- msv_multi_destroy)
    msvrt::Stream stream;
    ncclComm_t comm = nullptr;
    msvrt::CsrStaging staged;  // the shard's current chunk; d_scores: the whole shard's scores
};

}  // namespace

struct msv_multi {
    std::vector<Rank> ranks;
    DeviceBuffer<float> d_all;  // device 0: every score, input order
};

namespace {

// msv_debug_multi_no_alias: make pinned_alias fail, so the copy fallback below runs (tests).
std::atomic<bool> g_no_alias{false};

// Device alias of page-locked host residues (nullptr for pageable memory): every rank's kernel then
// reads its shard in place over its own PCIe link instead of a staged copy (as msv_score_batch does).
// Called with the rank's device current.  ROCm documents hipHostMallocPortable as its default behaviour
// (page-locked memory is registered for every device), which covers msv_host_alloc and torch pin_memory;
// whether a non-owning device gets an alias has only run on one-GPU boxes here, so it is not relied on:
// when the call fails, nullptr sends the shard through the copy path (enqueue_shard), which
// msv_debug_multi_no_alias forces in the GPU tests (bitwise against one launch).
const uint8_t* pinned_alias(const uint8_t* host) {
    if (!host || g_no_alias.load(std::memory_order_relaxed)) return nullptr;
    return msvrt::mapped_host(host);
}

// Upload shard [first, last) to rank r's device and enqueue its order + kernel launches on the rank's stream,
// one per chunk of < 4 GiB of residues and fewer than kMaxLaunchSeqs sequences (msv_plan.h plan_pieces;
// msv_profile_reserve_length has refused any sequence longer than a chunk).  Runs on the rank's own host
// thread; msv_multi_score_batch drains the stream before it returns.
msv_status enqueue_shard(Rank& r, const uint8_t* residues, const uint64_t* offsets, uint64_t first, uint64_t last) {
    DeviceGuard g(r.device);
    if (!g.ok) return MSV_ERR_NO_DEVICE;
    msvrt::CsrStaging& sg = r.staged;
    const uint64_t cn = last - first, total = offsets[last] - offsets[first];
    // (copied instead where the kernel would outrun the in-place reads: small models, large shards)
    const uint8_t* const zres = msvplan::in_place_wins(r.states, total) ? pinned_alias(residues) : nullptr;
    const std::vector<uint64_t> cut = msvplan::plan_pieces(offsets + first, cn, total, 0, 1);
    for (size_t k = 0; k + 1 < cut.size(); ++k) {
        const uint64_t a = first + cut[k], b = first + cut[k + 1], n = b - a, bytes = offsets[b] - offsets[a];
        MSV_HIP(sg.reserve_results(n, cn));
        MSV_HIP(sg.upload(residues, offsets, a, b, !zres, r.stream, r.stream));
        msv_status s = msv_order_longest_first(r.profile, sg.d_off, n, sg.d_order, r.stream);
        if (s != MSV_OK) return s;
        const bool in_place = zres && bytes;
        const uint8_t* src = in_place ? zres + offsets[a] : sg.d_res.get();
        s = (in_place ? msv_score_batch_host_residues : msv_score_batch_device)(
            r.profile, sg.readable(src, bytes), std::max<uint64_t>(bytes, 1), sg.d_off, n, sg.d_order,
            sg.d_scores + (a - first), r.stream);
        if (s != MSV_OK) return s;
        // the pinned offsets are rewritten by the next chunk: let this chunk's copy finish first
        if (b < last) MSV_HIP(hipStreamSynchronize(r.stream));
    }
    return MSV_OK;
}

}  // namespace

extern "C" {

// Diagnostic (tests): on = every later msv_multi_score_batch copies page-locked shards instead of reading
// them in place, as if the device alias were unavailable.  Not in msv.h.
msv_status msv_debug_multi_no_alias(int on) {
    g_no_alias.store(on != 0, std::memory_order_relaxed);
    return MSV_OK;
}

void msv_multi_destroy(msv_multi* m) {
    if (!m) return;
    for (Rank& r : m->ranks) {
        if (r.device < 0) continue;
        DeviceGuard g(r.device);
        if (r.stream) (void)hipStreamSynchronize(r.stream);
        if (r.comm) (void)ncclCommDestroy(r.comm);
        const Rank released = std::move(r);  // its buffers, then its stream, freed here under its device
    }
    if (!m->ranks.empty()) {
        DeviceGuard g(m->ranks[0].device);
        m->d_all.reset();
    }
    delete m;
}

msv_status msv_multi_create(msv_profile* const* profiles, uint32_t n_profiles, msv_multi** out) {
    if (!profiles || n_profiles == 0 || !out) return MSV_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    std::vector<int> devs(n_profiles);
    std::vector<uint32_t> states(n_profiles);
    for (uint32_t k = 0; k < n_profiles; ++k) {
        msv_kernel_info info;
        if (!profiles[k] || msv_profile_describe(profiles[k], &info) != MSV_OK) return MSV_ERR_INVALID_ARGUMENT;
        devs[k] = info.device;
        states[k] = info.model_length - 1;
        for (uint32_t j = 0; j < k; ++j)
            if (devs[j] == devs[k]) return MSV_ERR_INVALID_ARGUMENT;  // one RCCL rank per device
    }
    auto* m = new (std::nothrow) msv_multi;
    if (!m) return MSV_ERR_OUT_OF_MEMORY;
    m->ranks.resize(n_profiles);
    for (uint32_t k = 0; k < n_profiles; ++k) {
        Rank& r = m->ranks[k];
        r.profile = profiles[k];
        r.device = devs[k];
        r.states = states[k];
        DeviceGuard g(r.device);
        if (!g.ok || r.stream.create(hipStreamNonBlocking) != hipSuccess) {
            msv_multi_destroy(m);
            return MSV_ERR_NO_DEVICE;
        }
    }
    // one communicator per device, ranks in the order given (rank 0 = profiles[0]'s device)
    std::vector<ncclComm_t> comms(n_profiles);
    if (ncclCommInitAll(comms.data(), static_cast<int>(n_profiles), devs.data()) != ncclSuccess) {
        msv_multi_destroy(m);
        return MSV_ERR_RCCL;
    }
    for (uint32_t k = 0; k < n_profiles; ++k) m->ranks[k].comm = comms[k];
    *out = m;
    return MSV_OK;
}

msv_status msv_multi_score_batch(msv_multi* m, const uint8_t* residues, const uint64_t* offsets, uint64_t n,
                                 float* scores) {
    if (!m || (n && (!offsets || !scores))) return MSV_ERR_INVALID_ARGUMENT;
    if (n == 0) return MSV_OK;
    uint64_t maxL = 0, total = 0;
    msv_status s = msvrt::csr_extent(offsets, n, &maxL, &total);
    if (s != MSV_OK) return s;
    if (total && !residues) return MSV_ERR_INVALID_ARGUMENT;
    const uint32_t R = static_cast<uint32_t>(m->ranks.size());
    std::vector<uint64_t> b(R + 1);
    s = msv_shard_bounds(offsets, n, R, b.data());
    if (s != MSV_OK) return s;
    for (Rank& r : m->ranks) {
        s = msv_profile_reserve_length(r.profile, maxL);
        if (s != MSV_OK) return s;
    }
    {
        DeviceGuard g(m->ranks[0].device);
        if (!g.ok) return MSV_ERR_NO_DEVICE;
        MSV_HIP(m->d_all.reserve(n));
    }
    // Every return from here on first waits for every rank's stream (idle already on success): a chunk's copy
    // that reads a rank's pinned offsets, rewritten by the next call, may still be queued.
    struct DrainRanks {
        msv_multi* m;
        ~DrainRanks() {
            for (Rank& r : m->ranks) {
                DeviceGuard g(r.device);
                (void)hipStreamSynchronize(r.stream);
            }
        }
    } drain{m};
    // 1. every rank uploads its shard and enqueues order + kernel, concurrently (one thread each)
    std::vector<msv_status> st(R, MSV_OK);
    std::vector<std::thread> workers;
    for (uint32_t k = 0; k < R; ++k) {
        if (b[k + 1] == b[k]) continue;
        workers.emplace_back([&, k] { st[k] = enqueue_shard(m->ranks[k], residues, offsets, b[k], b[k + 1]); });
    }
    for (auto& w : workers) w.join();
    for (uint32_t k = 0; k < R; ++k)
        if (st[k] != MSV_OK) return st[k];
    // 2. one RCCL group: shard k's scores -> device 0's buffer at offset b[k] (exact counts).  The
    //    calls switch the current device per rank; the guard gives the caller's back.  (Across two or
    //    more devices this exchange has not run on hardware yet: the test box has one GPU, where the
    //    group is rank 0's self send/recv.)
    DeviceGuard caller_device(m->ranks[0].device);
    if (!caller_device.ok) return MSV_ERR_NO_DEVICE;
    MM_NCCL(ncclGroupStart());
    for (uint32_t k = 0; k < R; ++k) {
        const uint64_t cnt = b[k + 1] - b[k];
        if (!cnt) continue;
        Rank& r = m->ranks[k];
        if (hipSetDevice(r.device) != hipSuccess ||
            ncclSend(r.staged.d_scores, cnt, ncclFloat32, 0, r.comm, r.stream) != ncclSuccess ||
            hipSetDevice(m->ranks[0].device) != hipSuccess ||
            ncclRecv(m->d_all + b[k], cnt, ncclFloat32, static_cast<int>(k), m->ranks[0].comm,
                     m->ranks[0].stream) != ncclSuccess) {
            (void)ncclGroupEnd();
            return MSV_ERR_RCCL;
        }
    }
    MM_NCCL(ncclGroupEnd());
    // 3. one D2H from device 0, then each rank's latched kernel errors
    {
        DeviceGuard g(m->ranks[0].device);
        MSV_HIP(hipMemcpyAsync(scores, m->d_all, n * sizeof(float), hipMemcpyDeviceToHost, m->ranks[0].stream));
        MSV_HIP(hipStreamSynchronize(m->ranks[0].stream));
    }
    msv_status first = MSV_OK;  // every rank's bits are read and cleared (its stream waited for), the first reported
    for (Rank& r : m->ranks) {
        s = msv_profile_check(r.profile, r.stream);
        if (first == MSV_OK) first = s;
    }
    return first;
}

}  // extern "C"
