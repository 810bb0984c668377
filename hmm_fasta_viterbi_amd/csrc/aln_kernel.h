// aln_kernel.h -- device-side interface of the alignment stage, shared by aln_kernel.hip and the
// C-ABI layer (aln_device.cpp).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "dom_kernel.h"
#include "msv.h"

namespace alnk {

using domk::kArrays;
using domk::kLanes;
using domk::kRows;
using domk::kRowWords;
using domk::kScanSteps;

constexpr int kFillWaves = 4;  // waves per workgroup of the fill kernel
constexpr int kWalkBlock = 64;

// Arguments of the three wave-per-item kernels (seq_queue.h names the queue's fields).  The batch is the items'
// own: sequence s IS item s, its residues the envelope's.  An item's workspace starts at ws + base[s] (32-bit
// words; aln_host.h's aln_item_bytes states its four parts).
struct AlnArgs {
    const float2* etab;            // match odds  [20][S/2][64]
    const float2* itab;            // insert odds [20][S/2][64] (ISC variants only)
    const float2* ttab;            // Forward slot arrays (recording) / Backward slot arrays (Backward)
    const float* scan;             // [6][64] the launch's scan multipliers
    const uint32_t* gates;         // fill: [ceil(S/4)][64] gate bytes (aln_host.h's aln_gates)
    const uint8_t* residues;       // the items' residues, CSR
    const uint64_t* offsets;       // n + 1
    const uint32_t* select;        // the chunk's items
    const uint32_t* select_count;  // their count, a device word
    const uint32_t* lc;            // [n] the configured length of each item: lentab[lc[s]] are its loop / move
    const uint64_t* base;          // [n] first workspace word of each item
    const float2* lentab;          // [lentab_n] odds {loop, move} by length
    float* scores;                 // [n] envelope scores, nats (recording: written; Backward, fill: read)
    float* oa_scores;              // [n] fill: C(Le)
    uint32_t* ws;                  // the chunk's workspace
    uint32_t* counter;             // {dequeue head, workgroups that left}: zero on entry and exit
    uint32_t* errors;              // sticky error bits (msvk::kErr*)
    uint64_t n;
    uint32_t lentab_n;
    float tBM, tEC, tEJ;           // odds
    uint32_t open_EC, open_EJ;     // fill: tr_E_C / tr_E_J finite
};

// One compiled instantiation of the three kernels: the domain stage's family (S states per lane, match odds in
// LDS or read from L2, informative insert odds or none).
struct AlnVariant {
    int S;
    bool elds, isc;
    int waves;            // of the recording and the Backward kernel
    const void* fwd_fn;
    const void* bck_fn;
    const void* fill_fn;  // (one per S: kFillWaves waves)
    const char* name;
};
const AlnVariant* aln_variants(int* count);
const void* walk_fn();
hipError_t aln_launch(const void* fn, int waves, uint32_t blocks, const AlnArgs& args, hipStream_t stream);

// The walk, one item per thread over items lo .. hi-1.  Count pass (domains null): counts[2 (s - lo)], [.. + 1] =
// the item's domains and ops.  Place pass: the item's domains end at dom_off[s - lo + 1], its ops and op_pp at
// ops_off[s - lo + 1], written backwards; ops_begin counts from the chunk's first op.
struct WalkArgs {
    const uint32_t* ws;
    const uint64_t* base;
    const uint64_t* offsets;
    const float* scores;
    const float* oa_scores;
    const msv_aln_item* items;
    uint32_t lo, hi;
    uint32_t S;
    uint32_t* counts;
    const uint64_t* dom_off;
    const uint64_t* ops_off;
    msv_vit_domain* domains;
    uint8_t* ops;
    float* op_pp;
};
hipError_t launch_walk(const WalkArgs& a, hipStream_t stream);

}  // namespace alnk
