// emit_kernel.h -- device-side interface of the emit stage, shared by emit.hip and the C-ABI layer
// (emit_device.cpp).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "emit_host.h"
#include "msv.h"

namespace emitk {

constexpr int kWalkBlock = 64;    // one wave: a walk is serial and diverges from its neighbours' at the first draw
constexpr int kScanBlock = 1024;  // the scan's single workgroup

// The count and the place launch: one sequence per thread, sequence first + t at thread t < n.  Count writes
// counts[t]; place reads offsets[t], (with truth) domain_offsets[t] and the ops offset the scan left in counts[t], and
// returns at once where the scan's record says a total exceeded its capacity.
struct WalkArgs {
    msv_host::EmitConfig config;
    const uint32_t* match;   // [LENG + 1][19]
    const uint32_t* insert;  // [LENG + 1][19]
    const uint32_t* trans;   // [LENG + 1][4]
    msv_host::EmitCounts* counts;  // [n]; after the scan, words 0 and 1 hold the sequence's first op index
    const msv_emit_totals* record;
    const uint64_t* offsets;
    const uint64_t* domain_offsets;  // the truth buffers: all null without truth
    uint8_t* codes;
    msv_vit_domain* domains;
    uint8_t* ops;
    uint8_t* truncated;
    uint64_t seed, first, n;
};
hipError_t launch_count(const WalkArgs& a, hipStream_t stream);
hipError_t launch_place(const WalkArgs& a, hipStream_t stream);

// The scan launch: thread t of the one workgroup owns sequences [t per, (t + 1) per), per = ceil(n / 1024); sums
// them, the 1024 sums meet in an LDS scan, the totals and the overflow bits go to *record, and -- unless a total
// exceeds its capacity -- the thread writes its sequences' offsets (offsets[n] too) and turns each counts record into
// the sequence's first op index.
struct ScanArgs {
    msv_host::EmitCounts* counts;
    uint64_t* offsets;         // [n + 1]
    uint64_t* domain_offsets;  // [n + 1] or null
    msv_emit_totals* record;
    uint64_t n;
    uint64_t capacity, domains_capacity, ops_capacity;
};
hipError_t launch_scan(const ScanArgs& a, hipStream_t stream);

const void* count_fn();
const void* place_fn();
const void* scan_fn();

}  // namespace emitk
