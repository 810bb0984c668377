// spl_kernel.h -- device-side interface of the split stage, shared by spl_kernel.hip and the C-ABI
// layer (spl_device.cpp).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "dom_kernel.h"
#include "msv.h"

namespace splk {

// (the text of p7_kernel_head.inc and p7_forward_row.inc, included into spl_fwd_kernel, names all five unqualified)
using domk::kArrays;
using domk::kLanes;
using domk::kRows;
using domk::kRowWords;
using domk::kScanSteps;

constexpr int kSampleBlock = 64;  // one wave: consecutive samples of one item

// Arguments of the recording kernel (seq_queue.h names the queue's fields; alnk::AlnArgs names the rest alike).  The
// batch is the items' own: sequence s IS item s.  An item's workspace starts at ws + base[s] (32-bit words;
// spl_host.h's spl_item_bytes states its two parts).
struct SplArgs {
    const float2* etab;            // match odds  [20][S/2][64]
    const float2* itab;            // insert odds [20][S/2][64] (ISC variants only)
    const float2* ttab;            // Forward slot arrays
    const float* scan;             // [6][64] Forward's scan multipliers
    const uint8_t* residues;       // the items' residues, CSR
    const uint64_t* offsets;       // n + 1
    const uint32_t* select;        // the chunk's items
    const uint32_t* select_count;  // their count, a device word
    const uint32_t* lc;            // [n] the configured length of each item
    const uint64_t* base;          // [n] first workspace word of each item
    const float2* lentab;          // [lentab_n] odds {loop, move} by length
    float* scores;                 // [n] envelope scores, nats
    uint32_t* ws;                  // the chunk's workspace
    uint32_t* counter;             // {dequeue head, workgroups that left}: zero on entry and exit
    uint32_t* errors;              // sticky error bits (msvk::kErr*)
    uint64_t n;
    uint32_t lentab_n;
    float tBM, tEC, tEJ;           // odds
};

// One compiled instantiation of the recording kernel: the alignment stage's family.
struct SplVariant {
    int S;
    bool elds, isc;
    int waves;
    const void* fwd_fn;
    const char* name;
};
const SplVariant* spl_variants(int* count);
const void* sample_fn();
hipError_t spl_launch(const void* fn, int waves, uint32_t blocks, const SplArgs& args, hipStream_t stream);

// The sampler over items lo .. hi-1, one (item, sample) per thread, a wave's lanes consecutive samples of one item:
// workgroup b of ceil(n_samples / 64) per item.  Count pass (segments null): counts[(s - lo) n_samples + j] = the
// sample's domains, bit 31 set where it was truncated.  Place pass: the sample's segments end at
// seg_off[(s - lo) n_samples + j + 1], written backwards.
struct SampleArgs {
    const uint32_t* ws;
    const uint64_t* base;
    const uint64_t* offsets;
    const float* scores;
    const msv_aln_item* items;
    const uint32_t* lc;
    const float2* lentab;
    const float* tr;               // [LENG + 1][7] float32 transition odds (spl_host.h's spl_odds)
    uint32_t lo, hi;
    uint32_t S, leng, n_samples;
    float tBM, tEC, tEJ;
    uint64_t seed;
    uint32_t* counts;
    const uint64_t* seg_off;
    msv_spl_segment* segments;
};
hipError_t launch_sample(const SampleArgs& a, hipStream_t stream);

}  // namespace splk
