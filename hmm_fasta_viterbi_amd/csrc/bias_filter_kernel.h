// bias_filter_kernel.h -- device-side interface of the bias filter, shared by bias_filter.hip and the
// C-ABI layer (bias_filter_device.cpp).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace bfk {

constexpr int kWaves = 4;    // waves per workgroup, one sequence per wave
constexpr int kChunk = 16;   // consecutive residues of a lane per trip: one 16-byte load
constexpr int kTrip = 64 * kChunk;

struct BfArgs {
    const float* table;            // msv_host::kBfTableFloats: T, pi, r[20]
    const uint8_t* residues;       // CSR residue codes
    const uint64_t* offsets;       // n + 1
    const uint32_t* select;        // optional: the sequence indices to score (else 0 .. n-1)
    const uint32_t* select_count;  // optional device count of `select` entries (else n)
    float* scores;                 // the bias, written at the sequence index, nats
    uint32_t* counter;             // {dequeue head, workgroups that left}: zero on entry and exit
    uint32_t* errors;              // sticky error bits (msvk::kErr*)
    uint64_t n;
};

const void* bf_kernel();
hipError_t bf_launch(uint32_t blocks, const BfArgs& args, hipStream_t stream);

// vitk::launch_select with the bias term: the sequences with a filtered Gumbel P-value <= threshold, in `order`
// (else index order), stable; *count their number; pvalues optional.
hipError_t launch_bf_select(const float* scores, const float* bias, const uint64_t* offsets, const uint32_t* order,
                            uint64_t n, float mu, float lambda, double threshold, double* pvalues, uint32_t* select,
                            uint32_t* count, hipStream_t stream);
// Filtered P-values of n scores, lengths from the offsets: kind is msv.h's MSV_BF_GUMBEL / MSV_BF_EXPONENTIAL.
hipError_t launch_bf_pvalues(const float* scores, const float* bias, const uint64_t* offsets, uint64_t n,
                             float location, float scale, int kind, double* pvalues, hipStream_t stream);

}  // namespace bfk
