// vit_trace.h -- device-side interface of the Viterbi trace, shared by vit_trace.hip and the
// C-ABI layer (vit_trace_device.cpp).  The plans and the back-pointer layout are vit_trace_plan.h's.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "msv.h"

namespace vittrace {

// One fill launch: the chunk's `n_items` select entries, item j = sequence select[j] of the staged batch, its
// workspace (L rows of words x lanes back-pointers, then L row records) at ws + base[j] uint32.
struct FillArgs {
    const float2* etab;       // vit_tables of the plan's (S, team): match scores  [20][S/2][lanes] float2
    const float2* itab;       // insert scores, or nullptr (zero insert scores)
    const float2* ttab;       // transitions [7][S/2][lanes] float2
    const uint8_t* residues;
    const uint64_t* offsets;  // n + 1
    const uint32_t* select;   // n_items entries, each < n (checked on the host)
    const uint64_t* base;     // n_items
    const float2* lentab;     // [lentab_n] {tr_loop, tr_move}
    uint32_t* ws;
    float* scores;            // per item
    uint32_t* counter;        // {dequeue head, workgroups that left}: zero on entry and exit
    uint32_t* errors;
    uint32_t n_items;
    uint32_t lentab_n;
    float tr_B_Mk, tr_E_C, tr_E_J;
};

// The walk: one lane per item follows the pointers from C(L) back to N.  Pass 1 (domains == nullptr) writes
// counts[2j] = n_domains, counts[2j + 1] = n_ops; pass 2 writes the item's domains and ops backwards from the
// ends of its ranges [dom_off[j], dom_off[j+1]) and [ops_off[j], ops_off[j+1]) (ops_begin relative to `ops`).
struct WalkArgs {
    const uint64_t* offsets;
    const uint32_t* select;
    const uint64_t* base;
    const uint32_t* ws;
    const float* scores;
    uint32_t* counts;
    const uint64_t* dom_off;
    const uint64_t* ops_off;
    msv_vit_domain* domains;
    uint8_t* ops;
    uint32_t n_items;
    uint32_t S, words, lanes;
};

const void* fill_kernel(int plan);  // vit_trace_plan.h's kPlans[plan]
hipError_t launch_fill(int plan, uint32_t blocks, const FillArgs& a, hipStream_t stream);
hipError_t launch_walk(const WalkArgs& a, hipStream_t stream);

}  // namespace vittrace
