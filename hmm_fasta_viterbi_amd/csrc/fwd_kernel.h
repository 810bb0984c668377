// fwd_kernel.h -- device-side interface of the Forward stage, shared by fwd_kernel.hip and the
// C-ABI layer (fwd_device.cpp).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace fwdk {

constexpr int kRows = 20;      // residue rows of the odds tables (codes >= 20 are flagged, not scored)
constexpr int kArrays = 8;     // per-slot arrays of FwdArgs::ttab: vit_kernel.h's 7 transitions, then DC
constexpr int kLanes = 64;     // one sequence per wave
constexpr int kScanSteps = 6;  // log2(kLanes) steps of the D chain's cross-lane scan

// Slot arrays (odds, 0 where the transition does not exist), per lane slot q (state k = lane * S + q + 1):
// as vitk::MM_IN .. DD_IN, then DC: c_q = tDD(slot 0) * .. * tDD(slot q), the D-scan's fix-up multipliers.
enum : int { MM_IN = 0, IM_IN = 1, DM_IN = 2, MI = 3, II = 4, MD_IN = 5, DD_IN = 6, DC = 7 };

struct FwdArgs {
    const float2* etab;            // match odds  [20][S/2][64] float2 (padding slots 0)
    const float2* itab;            // insert odds [20][S/2][64] float2 (ISC variants only)
    const float2* ttab;            // slot arrays [8][S/2][64] float2
    const float* scan;             // [6][64] the scan steps' lane multipliers (fwd_host.h)
    const uint8_t* residues;       // CSR residue codes
    const uint64_t* offsets;       // n + 1
    const uint32_t* select;        // optional: the sequence indices to score (else 0 .. n-1)
    const uint32_t* select_count;  // optional device count of `select` entries (else n)
    const float2* lentab;          // [lentab_n] odds {loop, move} by length
    float* scores;                 // written at the sequence index, nats
    uint32_t* counter;             // {dequeue head, workgroups that left}: zero on entry and exit
    uint32_t* errors;              // sticky error bits (msvk::kErr*)
    uint64_t n;
    uint32_t lentab_n;
    float tBM, tEC, tEJ;           // odds
};

// One compiled instantiation: S states per lane (covers 64 * S states), match odds staged in LDS (elds) or
// read from L2 every row, informative insert odds (isc, read from L2) or none; `waves` waves per workgroup.
// One variant per S and insert mode: every one is the automatic choice for its band.
struct FwdVariant {
    int S;
    bool elds, isc;
    int waves;
    const void* fn;
    const char* name;
    int states() const { return kLanes * S; }
};

const FwdVariant* fwd_variants(int* count);
hipError_t fwd_launch(const FwdVariant& v, uint32_t blocks, const FwdArgs& args, hipStream_t stream);
// Forward P-values (fwd_pvalue_of) of n scores; lengths from the offsets.
hipError_t launch_fwd_pvalues(const float* scores, const uint64_t* offsets, uint64_t n, float tau, float lambda,
                              double* pvalues, hipStream_t stream);

}  // namespace fwdk
