// emit_device.cpp -- C-ABI of the emit stage (msv.h "Emit stage") on the HIP runtime.
//
// The handle owns the uploaded threshold tables, the counts records of the call under way, the totals record with
// its pinned host copy and, for msv_emit_batch, the chunk's output buffers.  A call enqueues the count, the scan and
// the place launch on the caller's stream and waits for it once, to read the totals back; msv_emit_batch waits
// between the scan and the place launch instead, because the totals size the chunk's buffers.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <limits>
#include <memory>
#include <new>

#include "emit_host.h"
#include "emit_kernel.h"
#include "hip_rt.h"
#include "host_cpu.h"
#include "msv.h"

using msvrt::DeviceBuffer;
using msvrt::DeviceGuard;
using msv_host::EmitCounts;

static_assert(msv_host::kEmitMaxResidues == msvrt::kChunkBytes, "a device call emits what the engines take");
static_assert(sizeof(EmitCounts) == 16 && sizeof(msv_vit_domain) == 32, "records as the kernels store them");

struct msv_emit_profile {
    int device = 0;
    msv_host::EmitTables tables;
    DeviceBuffer<uint32_t> d_match, d_insert, d_trans;
    DeviceBuffer<EmitCounts> d_counts;
    DeviceBuffer<msv_emit_totals> d_record;
    msvrt::PinnedBuffer<msv_emit_totals> h_record;
    DeviceBuffer<uint8_t> d_fixed, d_var;  // msv_emit_batch: a chunk's offsets and flags; its codes, domains and ops
    msvrt::Stream own;
    hipStream_t bound = nullptr;
    msvrt::Event ev[5];  // 0-1 around the count launch, 1-2 around the scan, 3-4 around the place launch
    float ms[3] = {0, 0, 0};  // device times of the last call's launches, summed over its chunks
};

namespace {

constexpr uint64_t kNoCapacity = std::numeric_limits<uint64_t>::max();

emitk::WalkArgs walk_args(const msv_emit_profile* p, uint64_t seed, uint64_t first, uint64_t n) {
    emitk::WalkArgs a{};
    a.config = p->tables.config;
    a.match = p->d_match;
    a.insert = p->d_insert;
    a.trans = p->d_trans;
    a.counts = p->d_counts;
    a.record = p->d_record;
    a.seed = seed;
    a.first = first;
    a.n = n;
    return a;
}

// The count and the scan launch of sequences first .. first + n - 1, and the copy of the totals into h_record.
msv_status enqueue_count_scan(msv_emit_profile* p, uint64_t seed, uint64_t first, uint64_t n, uint64_t* d_offsets,
                              const msv_emit_truth* truth, uint64_t capacity, hipStream_t st) {
    MSV_HIP(p->d_counts.reserve(n));
    const emitk::WalkArgs w = walk_args(p, seed, first, n);
    MSV_HIP(hipEventRecord(p->ev[0], st));
    MSV_HIP(emitk::launch_count(w, st));
    MSV_HIP(hipEventRecord(p->ev[1], st));
    emitk::ScanArgs s{};
    s.counts = p->d_counts;
    s.offsets = d_offsets;
    s.domain_offsets = truth ? truth->d_domain_offsets : nullptr;
    s.record = p->d_record;
    s.n = n;
    s.capacity = capacity;
    s.domains_capacity = truth ? truth->domains_capacity : 0;
    s.ops_capacity = truth ? truth->ops_capacity : 0;
    MSV_HIP(emitk::launch_scan(s, st));
    MSV_HIP(hipEventRecord(p->ev[2], st));
    MSV_HIP(hipMemcpyAsync(p->h_record, p->d_record, sizeof(msv_emit_totals), hipMemcpyDeviceToHost, st));
    return MSV_OK;
}

msv_status enqueue_place(msv_emit_profile* p, uint64_t seed, uint64_t first, uint64_t n, uint8_t* d_codes,
                         const uint64_t* d_offsets, const msv_emit_truth* truth, hipStream_t st) {
    emitk::WalkArgs w = walk_args(p, seed, first, n);
    w.offsets = d_offsets;
    w.codes = d_codes;
    if (truth) {
        w.domain_offsets = truth->d_domain_offsets;
        w.domains = truth->d_domains;
        w.ops = truth->d_ops;
        w.truncated = truth->d_truncated;
    }
    MSV_HIP(hipEventRecord(p->ev[3], st));
    MSV_HIP(emitk::launch_place(w, st));
    MSV_HIP(hipEventRecord(p->ev[4], st));
    return MSV_OK;
}

// Adds the device time between two recorded events, after the stream is done.
void add_ms(msv_emit_profile* p, int kind, int from) {
    p->ms[kind] += msvrt::elapsed(p->ev[from], p->ev[from + 1]);
}

bool truth_ok(const msv_emit_truth* t, uint64_t n) {
    if (!t) return true;
    if (!t->d_domain_offsets || (n && !t->d_truncated)) return false;
    if ((t->domains_capacity && !t->d_domains) || (t->ops_capacity && !t->d_ops)) return false;
    return reinterpret_cast<uintptr_t>(t->d_domain_offsets) % 8 == 0 &&
           reinterpret_cast<uintptr_t>(t->d_domains) % 8 == 0;
}

template <class T>
T* carve(uint8_t*& at, uint64_t bytes) {
    T* const out = reinterpret_cast<T*>(at);
    at += msv_host::emit_round16(bytes);
    return out;
}

}  // namespace

extern "C" {

msv_status msv_emit_profile_create(int device, const msv_hmm* hmm, const msv_emit_options* options,
                                   msv_emit_profile** out) try {
    if (!hmm || !out) return MSV_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    msv_host::EmitTables tables;
    const msv_status s = msv_host::emit_tables(hmm, options, &tables);
    if (s != MSV_OK) return s;
    DeviceGuard g(device);
    if (!g.ok) return MSV_ERR_NO_DEVICE;
    std::unique_ptr<msv_emit_profile> guard(new msv_emit_profile);
    msv_emit_profile* const p = guard.get();
    p->device = device;
    p->tables = std::move(tables);
    MSV_HIP(p->d_match.replace_with(p->tables.match.data(), p->tables.match.size()));
    MSV_HIP(p->d_insert.replace_with(p->tables.insert.data(), p->tables.insert.size()));
    MSV_HIP(p->d_trans.replace_with(p->tables.trans.data(), p->tables.trans.size()));
    MSV_HIP(p->d_record.reserve(1));
    MSV_HIP(p->h_record.reserve(1));
    MSV_HIP(p->own.create(hipStreamNonBlocking));
    for (auto& e : p->ev) MSV_HIP(e.create(hipEventDefault));
    *out = guard.release();
    return MSV_OK;
} catch (const std::bad_alloc&) {
    return MSV_ERR_OUT_OF_MEMORY;
}

void msv_emit_profile_destroy(msv_emit_profile* p) {
    if (!p) return;
    DeviceGuard g(p->device);
    (void)hipStreamSynchronize(p->own);
    delete p;
}

msv_status msv_emit_profile_bind_stream(msv_emit_profile* p, void* stream) {
    if (!p) return MSV_ERR_INVALID_ARGUMENT;
    p->bound = static_cast<hipStream_t>(stream);
    return MSV_OK;
}

msv_status msv_emit_batch_device(msv_emit_profile* p, uint64_t seed, uint64_t first, uint64_t n, uint8_t* d_codes,
                                 uint64_t capacity, uint64_t* d_offsets, const msv_emit_truth* truth,
                                 msv_emit_totals* totals, void* stream) {
    if (!p || !stream || !d_offsets || reinterpret_cast<uintptr_t>(d_offsets) % 8 || (capacity && !d_codes) ||
        n >= msvrt::kMaxLaunchSeqs || !truth_ok(truth, n))
        return MSV_ERR_INVALID_ARGUMENT;
    DeviceGuard g(p->device);
    if (!g.ok) return MSV_ERR_NO_DEVICE;
    const hipStream_t st = static_cast<hipStream_t>(stream);
    msvrt::StreamDrain drain(st);
    p->ms[0] = p->ms[1] = p->ms[2] = 0.0f;
    msv_status s = enqueue_count_scan(p, seed, first, n, d_offsets, truth, capacity, st);
    if (s != MSV_OK) return s;
    if ((s = enqueue_place(p, seed, first, n, d_codes, d_offsets, truth, st)) != MSV_OK) return s;
    MSV_HIP(hipStreamSynchronize(st));
    drain.disarm();
    add_ms(p, 0, 0);
    add_ms(p, 1, 1);
    add_ms(p, 2, 3);
    if (totals) *totals = *p->h_record.get();
    return p->h_record.get()->overflow ? MSV_ERR_OUT_OF_MEMORY : MSV_OK;
}

msv_status msv_emit_batch(msv_emit_profile* p, uint64_t seed, uint64_t first, uint64_t n, int truth,
                          uint64_t workspace_bytes, void* stream, msv_emit_result** result) try {
    if (!p || !result) return MSV_ERR_INVALID_ARGUMENT;
    *result = nullptr;
    if (n >= (1ull << 32)) return MSV_ERR_INVALID_ARGUMENT;
    const bool tr = truth != 0;
    const uint64_t budget = workspace_bytes ? workspace_bytes : msv_host::kEmitDefaultWorkspace;
    DeviceGuard g(p->device);
    if (!g.ok) return MSV_ERR_NO_DEVICE;
    const hipStream_t st = stream     ? static_cast<hipStream_t>(stream)
                           : p->bound ? p->bound
                                      : static_cast<hipStream_t>(p->own);

    std::unique_ptr<msv_emit_result> guard(new msv_emit_result);
    msv_emit_result* const r = guard.get();
    r->truth = tr;
    r->offsets.assign(n + 1, 0);
    r->domain_offsets.assign(n + 1, 0);
    r->truncated.assign(n, 0);

    msvrt::StreamDrain drain(st);
    p->ms[0] = p->ms[1] = p->ms[2] = 0.0f;
    uint64_t m = std::min<uint64_t>(std::max<uint64_t>(n, 1), msvrt::kMaxLaunchSeqs - 1);
    for (uint64_t done = 0; done < n;) {
        m = std::min(m, n - done);
        // the chunk's fixed part: offsets, domain offsets and flags (the counts records are the handle's)
        if (msv_host::emit_fixed_bytes(m, tr) > budget) {
            if (m == 1) return MSV_ERR_OUT_OF_MEMORY;
            m /= 2;
            continue;
        }
        MSV_HIP(p->d_fixed.reserve(msv_host::emit_fixed_bytes(m, tr) - 16 * m));
        uint8_t* at = p->d_fixed;
        msv_emit_truth t{};
        uint64_t* const d_off = carve<uint64_t>(at, 8 * (m + 1));
        if (tr) {
            t.d_domain_offsets = carve<uint64_t>(at, 8 * (m + 1));
            t.d_truncated = carve<uint8_t>(at, m);
            t.domains_capacity = t.ops_capacity = kNoCapacity;
        }
        msv_status s = enqueue_count_scan(p, seed, first + done, m, d_off, tr ? &t : nullptr, kNoCapacity, st);
        if (s != MSV_OK) return s;
        MSV_HIP(hipStreamSynchronize(st));
        add_ms(p, 0, 0);
        add_ms(p, 1, 1);
        const msv_emit_totals tot = *p->h_record.get();
        if (tot.overflow || msv_host::emit_workspace_bytes(m, tot.residues, tot.domains, tot.ops, tr) > budget) {
            if (m == 1) return MSV_ERR_OUT_OF_MEMORY;
            m /= 2;
            continue;
        }
        MSV_HIP(p->d_var.reserve(msv_host::emit_workspace_bytes(m, tot.residues, tot.domains, tot.ops, tr) -
                                 msv_host::emit_fixed_bytes(m, tr)));
        at = p->d_var;
        uint8_t* const d_codes = carve<uint8_t>(at, tot.residues);
        if (tr) {
            t.d_domains = carve<msv_vit_domain>(at, tot.domains * sizeof(msv_vit_domain));
            t.d_ops = carve<uint8_t>(at, tot.ops);
        }
        if ((s = enqueue_place(p, seed, first + done, m, d_codes, d_off, tr ? &t : nullptr, st)) != MSV_OK) return s;

        const uint64_t c0 = r->codes.size(), d0 = r->domains.size(), o0 = r->ops.size();
        r->codes.resize(c0 + tot.residues);
        if (tot.residues)
            MSV_HIP(hipMemcpyAsync(r->codes.data() + c0, d_codes, tot.residues, hipMemcpyDeviceToHost, st));
        MSV_HIP(hipMemcpyAsync(r->offsets.data() + done + 1, d_off + 1, 8 * m, hipMemcpyDeviceToHost, st));
        if (tr) {
            r->domains.resize(d0 + tot.domains);
            r->ops.resize(o0 + tot.ops);
            MSV_HIP(hipMemcpyAsync(r->domain_offsets.data() + done + 1, t.d_domain_offsets + 1, 8 * m,
                                   hipMemcpyDeviceToHost, st));
            MSV_HIP(hipMemcpyAsync(r->truncated.data() + done, t.d_truncated, m, hipMemcpyDeviceToHost, st));
            if (tot.domains)
                MSV_HIP(hipMemcpyAsync(r->domains.data() + d0, t.d_domains, tot.domains * sizeof(msv_vit_domain),
                                       hipMemcpyDeviceToHost, st));
            if (tot.ops) MSV_HIP(hipMemcpyAsync(r->ops.data() + o0, t.d_ops, tot.ops, hipMemcpyDeviceToHost, st));
        }
        MSV_HIP(hipStreamSynchronize(st));  // the next chunk rewrites the buffers
        add_ms(p, 2, 3);
        for (uint64_t j = done + 1; j <= done + m; ++j) {
            r->offsets[j] += c0;
            r->domain_offsets[j] += d0;
        }
        for (uint64_t q = d0; q < r->domains.size(); ++q) {
            r->domains[q].seq += static_cast<uint32_t>(done);
            r->domains[q].ops_begin += o0;
        }
        r->chunks += 1;
        done += m;
    }
    drain.disarm();
    *result = guard.release();
    return MSV_OK;
} catch (const std::bad_alloc&) {
    return MSV_ERR_OUT_OF_MEMORY;
}

msv_status msv_emit_profile_times(const msv_emit_profile* p, float* count_ms, float* scan_ms, float* place_ms) {
    if (!p) return MSV_ERR_INVALID_ARGUMENT;
    if (count_ms) *count_ms = p->ms[0];
    if (scan_ms) *scan_ms = p->ms[1];
    if (place_ms) *place_ms = p->ms[2];
    return MSV_OK;
}

msv_status msv_emit_describe(const msv_emit_profile* p, msv_emit_info* out) {
    if (!p || !out || out->struct_size < sizeof(uint32_t)) return MSV_ERR_INVALID_ARGUMENT;
    DeviceGuard g(p->device);
    if (!g.ok) return MSV_ERR_NO_DEVICE;
    msv_emit_info info;
    std::memset(&info, 0, sizeof(info));
    info.model_length = p->tables.model_length;
    info.block = emitk::kWalkBlock;
    info.scan_block = emitk::kScanBlock;
    msvrt::kernel_footprint(emitk::count_fn(), &info.count_scratch_bytes, &info.count_lds_bytes, &info.count_vgprs);
    msvrt::kernel_footprint(emitk::place_fn(), &info.place_scratch_bytes, &info.place_lds_bytes, &info.place_vgprs);
    msvrt::kernel_footprint(emitk::scan_fn(), &info.scan_scratch_bytes, &info.scan_lds_bytes, &info.scan_vgprs);
    info.device = p->device;
    info.table_bytes = p->tables.bytes();
    info.length = p->tables.length;
    info.max_length = p->tables.config.max_length;
    info.unihit = p->tables.config.multihit ? 0 : 1;
    info.insert_mode = p->tables.config.file_inserts ? MSV_INSERTS_LOG_ODDS : MSV_INSERTS_ZERO;
    info.default_workspace_bytes = msv_host::kEmitDefaultWorkspace;
    msv_host::write_sized(out, info);
    return MSV_OK;
}

}  // extern "C"
