// aln_null2.h -- device-side interface of the bias stage, shared by aln_null2.hip and the C-ABI layer
// (aln_device.cpp).  The two kernels only read the alignment workspace (aln_host.h's layout) after Backward.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace alnk {

constexpr int kNull2Waves = 4;  // waves per workgroup of both kernels

struct Null2Args {
    const uint32_t* ws;          // the chunk's workspace
    const uint64_t* base;        // [n] first workspace word of each item
    const uint64_t* offsets;     // n + 1, the items' own CSR: Le of item s
    const float* scores;         // [n] envelope scores: an item whose score is not finite is skipped
    const uint32_t* unit_item;   // [units] the item of each of the chunk's units
    const uint32_t* unit_first;  // [n] the first unit of each item, counted from its chunk's first
    float* slabs;                // [units][2 S + 1][64]
    const float2* etab;          // match odds  [20][S/2][64]
    const float2* itab;          // insert odds [20][S/2][64] (ISC variants only)
    float* null2;                // [n][20]
    uint32_t units;              // of the chunk
    uint32_t lo, hi;             // the chunk's items
    uint32_t leng;               // LENG
};

struct Null2Variant {
    int S;
    bool isc;
    const void* partial_fn;  // (one per S)
    const void* finish_fn;
};
const Null2Variant* null2_variant(int S, bool isc);
// One wave per unit, then one wave per item of lo .. hi-1; plain grids (no queue: the units are alike).
hipError_t null2_launch_partial(const Null2Variant* v, const Null2Args& a, hipStream_t stream);
hipError_t null2_launch_finish(const Null2Variant* v, const Null2Args& a, hipStream_t stream);

}  // namespace alnk
