// dom_kernel.h -- device-side interface of the domain stage, shared by dom_kernel.hip and the
// C-ABI layer (dom_device.cpp).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "fwd_kernel.h"
#include "msv.h"

namespace domk {

using fwdk::kArrays;     // per-slot arrays of ttab (fwd_kernel.h's) and of btab (below)
using fwdk::kLanes;
using fwdk::kRows;
using fwdk::kScanSteps;  // steps of either D chain's cross-lane scan
constexpr int kRowWords = 6;   // a Forward record: N, J, C, B, E (float bits) and the running exponent (int32)

// Backward slot arrays (odds, 0 where the transition does not exist), per lane slot q (state k = lane * S + q + 1):
// the seven transitions OUT of node k, then SFX: s_q = tDD(slot q) * .. * tDD(slot S-1), the mirrored D-scan's
// fix-up multipliers.
enum : int { B_MM = 0, B_MI = 1, B_MD = 2, B_IM = 3, B_II = 4, B_DM = 5, B_DD = 6, B_SFX = 7 };

// Arguments of both kernels (seq_queue.h names the queue's fields).  `scores` is the launch's own score array:
// the recording kernel's Forward scores, the Backward kernel's Backward scores.
struct DomArgs {
    const float2* etab;            // match odds  [20][S/2][64] float2 (padding slots 0)
    const float2* itab;            // insert odds [20][S/2][64] float2 (ISC variants only)
    const float2* ttab;            // Forward slot arrays [8][S/2][64] (recording) / Backward slot arrays (Backward)
    const float* scan;             // [6][64] the launch's scan multipliers
    const uint8_t* residues;       // CSR residue codes
    const uint64_t* offsets;       // n + 1
    const uint32_t* select;        // optional: the sequence indices (else 0 .. n-1)
    const uint32_t* select_count;  // optional device count of `select` entries (else n)
    const uint64_t* item_rows;     // optional: list entry -> its first workspace row (else offsets[s] + s)
    const float2* lentab;          // [lentab_n] odds {loop, move} by length
    float* scores;                 // written at the sequence index, nats
    const float* fwd_scores;       // Backward: the recording launch's scores (a non-finite one: sequence skipped)
    uint32_t* records;             // workspace rows of kRowWords words (recording: written, null = none; Backward: read)
    float* begin;                  // Backward: per-residue outputs at the residue's CSR index
    float* end;
    float* occ;
    uint32_t* counter;             // {dequeue head, workgroups that left}: zero on entry and exit
    uint32_t* errors;              // sticky error bits (msvk::kErr*)
    uint64_t n;
    uint32_t lentab_n;
    float tBM, tEC, tEJ;           // odds
};

// One compiled instantiation of the pair of kernels, Forward's family: S states per lane, match odds in LDS
// (elds) or read from L2, informative insert odds (isc) or none; `waves` waves per workgroup.
struct DomVariant {
    int S;
    bool elds, isc;
    int waves;
    const void* fn;      // dom_fwd_kernel (the occupancy of `blocks`)
    const void* bck_fn;  // dom_bck_kernel
    const char* name;
    int states() const { return kLanes * S; }
};

const DomVariant* dom_variants(int* count);
hipError_t dom_launch(const void* fn, int waves, uint32_t blocks, const DomArgs& args, hipStream_t stream);

// The envelope rule (dom_host.h's dom_regions_scan), one list entry per thread.  counts[q] = regions of entry q
// (0 unless the entry's Forward score is finite); an exclusive scan (region_offsets[m + 1]); the records.
struct RegionArgs {
    const uint64_t* offsets;
    const uint32_t* select;  // optional
    const float* fwd_scores;
    const float* begin;
    const float* end;
    const float* occ;
    uint64_t n, m;           // sequences of the batch, list entries
    float rt1, rt2;
};
hipError_t launch_regions_count(const RegionArgs& a, uint32_t* counts, hipStream_t stream);
hipError_t launch_regions_scan(const uint32_t* counts, uint64_t m, uint64_t* region_offsets, hipStream_t stream);
hipError_t launch_regions_place(const RegionArgs& a, const uint64_t* region_offsets, msv_dom_region* regions,
                                hipStream_t stream);

}  // namespace domk
