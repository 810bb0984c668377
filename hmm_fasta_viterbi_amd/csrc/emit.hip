// emit.hip -- the emit stage on gfx950 (msv.h "Emit stage"): sequences drawn from the profile.
//
//   emit_count_kernel   one sequence per thread: emit_host.h's emit_walk, the function msv_emit_generate runs, into a
//                       sink that stores nothing; the thread writes its 16-byte counts record (length, domains, ops,
//                       truncated) with one vector store.  Integers only, so the counters are the host's.
//   emit_scan_kernel    ONE workgroup of kScanBlock = 1024 threads: thread t sums its contiguous run of records, the
//                       1024 sums meet in an LDS scan (ten doubling steps, no atomics), thread 0 writes the totals
//                       record with the overflow bits, and unless one is set every thread writes its run's uint64
//                       offsets and leaves each sequence's first op index in its counts record.
//   emit_place_kernel   the same walk with the same counters into a sink that stores codes, ops and domains at the
//                       scanned offsets: plain byte stores for codes and ops, one record store per domain.  It
//                       returns before any store where the scan's record carries an overflow bit.
//
// The tables (match and insert rows of 19 thresholds, 4 transition thresholds per node) are read from global memory:
// under 400 KiB at LENG 2,432, read-only and L2-resident; a residue's code is the 19-way count over its row (19
// independent loads, one latency), a transition draw one 16-byte load.  The background's thresholds and the
// configuration are kernel arguments.
#include <hip/hip_runtime.h>

#include "emit_host.h"
#include "emit_kernel.h"

namespace emitk {

using msv_host::EmitCounts;

__global__ __launch_bounds__(kWalkBlock) void emit_count_kernel(const WalkArgs a) {
    const uint64_t t = static_cast<uint64_t>(blockIdx.x) * kWalkBlock + threadIdx.x;
    if (t >= a.n) return;
    msv_host::EmitCountSink sink;
    const EmitCounts c =
        msv_host::emit_walk(a.config, a.match, a.insert, a.trans, msv_host::emit_key(a.seed, a.first + t), sink);
    *reinterpret_cast<uint4*>(a.counts + t) = make_uint4(c.length, c.domains, c.ops, c.truncated);
}

__global__ __launch_bounds__(kWalkBlock) void emit_place_kernel(const WalkArgs a) {
    const uint64_t t = static_cast<uint64_t>(blockIdx.x) * kWalkBlock + threadIdx.x;
    if (t >= a.n || a.record->overflow != 0) return;
    const uint2 first_op = *reinterpret_cast<const uint2*>(a.counts + t);
    const uint64_t op0 = static_cast<uint64_t>(first_op.x) | static_cast<uint64_t>(first_op.y) << 32;
    const bool truth = a.domain_offsets != nullptr;
    msv_host::EmitPlaceSink sink;
    sink.codes = a.codes + a.offsets[t];
    sink.domains = truth ? a.domains + a.domain_offsets[t] : nullptr;
    sink.ops = truth ? a.ops + op0 : nullptr;
    sink.seq = static_cast<uint32_t>(t);
    sink.ops_begin = op0;
    const EmitCounts c =
        msv_host::emit_walk(a.config, a.match, a.insert, a.trans, msv_host::emit_key(a.seed, a.first + t), sink);
    if (truth) a.truncated[t] = static_cast<uint8_t>(c.truncated);
}

__global__ __launch_bounds__(kScanBlock) void emit_scan_kernel(const ScanArgs a) {
    __shared__ uint64_t sh[4][kScanBlock];
    const uint32_t t = threadIdx.x;
    const uint64_t per = (a.n + kScanBlock - 1) / kScanBlock;
    const uint64_t lo = t * per < a.n ? t * per : a.n;
    const uint64_t hi = lo + per < a.n ? lo + per : a.n;
    uint64_t own[4] = {0, 0, 0, 0};
    for (uint64_t i = lo; i < hi; ++i) {
        const uint4 c = *reinterpret_cast<const uint4*>(a.counts + i);
        own[0] += c.x;
        own[1] += c.y;
        own[2] += c.z;
        own[3] += c.w;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) sh[q][t] = own[q];
    __syncthreads();
    for (uint32_t d = 1; d < kScanBlock; d <<= 1) {
        uint64_t v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = t >= d ? sh[q][t - d] : 0;
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 4; ++q) sh[q][t] += v[q];
        __syncthreads();
    }
    const uint64_t residues = sh[0][kScanBlock - 1], domains = sh[1][kScanBlock - 1], ops = sh[2][kScanBlock - 1];
    const bool truth = a.domain_offsets != nullptr;
    uint64_t overflow = 0;
    if (residues > a.capacity || residues >= msv_host::kEmitMaxResidues) overflow |= 1;
    if (truth && domains > a.domains_capacity) overflow |= 2;
    if (truth && ops > a.ops_capacity) overflow |= 4;
    if (t == 0) {
        msv_emit_totals r;
        r.residues = residues;
        r.domains = domains;
        r.ops = ops;
        r.truncated = sh[3][kScanBlock - 1];
        r.overflow = overflow;
        *a.record = r;
    }
    if (overflow) return;
    uint64_t at[3] = {sh[0][t] - own[0], sh[1][t] - own[1], sh[2][t] - own[2]};
    for (uint64_t i = lo; i < hi; ++i) {
        const uint4 c = *reinterpret_cast<const uint4*>(a.counts + i);
        a.offsets[i] = at[0];
        if (truth) a.domain_offsets[i] = at[1];
        *reinterpret_cast<uint2*>(a.counts + i) =
            make_uint2(static_cast<uint32_t>(at[2]), static_cast<uint32_t>(at[2] >> 32));
        at[0] += c.x;
        at[1] += c.y;
        at[2] += c.z;
    }
    if (t == 0) {
        a.offsets[a.n] = residues;
        if (truth) a.domain_offsets[a.n] = domains;
    }
}

namespace {

hipError_t launch_walk(const void* fn, const WalkArgs& a, hipStream_t stream) {
    const uint64_t blocks = (a.n + kWalkBlock - 1) / kWalkBlock;
    if (blocks == 0) return hipSuccess;
    if (blocks >= (1ull << 31)) return hipErrorInvalidValue;
    void* params[] = {const_cast<WalkArgs*>(&a)};
    return hipLaunchKernel(fn, dim3(static_cast<uint32_t>(blocks)), dim3(kWalkBlock), params, 0, stream);
}

}  // namespace

const void* count_fn() { return reinterpret_cast<const void*>(&emit_count_kernel); }
const void* place_fn() { return reinterpret_cast<const void*>(&emit_place_kernel); }
const void* scan_fn() { return reinterpret_cast<const void*>(&emit_scan_kernel); }

hipError_t launch_count(const WalkArgs& a, hipStream_t stream) { return launch_walk(count_fn(), a, stream); }
hipError_t launch_place(const WalkArgs& a, hipStream_t stream) { return launch_walk(place_fn(), a, stream); }

hipError_t launch_scan(const ScanArgs& a, hipStream_t stream) {
    void* params[] = {const_cast<ScanArgs*>(&a)};
    return hipLaunchKernel(scan_fn(), dim3(1), dim3(kScanBlock), params, 0, stream);
}

}  // namespace emitk
