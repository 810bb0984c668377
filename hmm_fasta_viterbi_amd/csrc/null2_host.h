// null2_host.h -- host-only half of the bias stage (msv.h "Bias stage"): the null2 model of an envelope
// "by expectation" in float64, THE definition of the correction from a float32 null2 vector (the batch call runs it on
// the device's vector, so the device's domcorrection has its bits), the bias / bit score / P-value arithmetic, and the
// row-block arithmetic the kernels of aln_null2.hip and the device layer share.  No HIP include: null2_host.cpp is
// built by plain g++ and runs under the sanitizers (tests/cpp/sanitize_null2.cpp).
#pragma once

#include <cstddef>
#include <cstdint>

#include "fwd_host.h"
#include "msv.h"

namespace msv_host {

constexpr uint64_t kNull2Residues = 20;
// R: the rows of one work unit of aln_null2_partial.  A compile-time constant of the kernels; the float32 order of
// summation is a function of (S, Le, R) only.
constexpr uint64_t kNull2RowBlock = 16;
constexpr double kNull2Omega = 1.0 / 256.0;

constexpr uint64_t null2_blocks(uint64_t Le) { return (Le + kNull2RowBlock - 1) / kNull2RowBlock; }
// One unit's slab: 2 S + 1 rows of 64 floats (eM by slot, eI by slot, then the lanes' shares of eX).
constexpr uint64_t null2_slab_floats(uint64_t S) { return (2 * S + 1) * 64; }

// The float64 null2 of an envelope (msv.h): the float64 decode, the expected emissions of every state, the weighted
// mean with the float32 odds the device tables hold.  null2 double [20]; *domcorrection in nats.  Le >= 1.
void null2_on_envelope(const FwdModel& m, const float* msc, const float* isc, const uint8_t* codes, size_t Le, size_t Lc,
                       double* null2, double* domcorrection);

// THE definition of the correction: n_x = the count of x among the Le codes; sum_x n_x log((double) null2[x]) in
// float64 for x = 0 .. 19 in that order, terms with n_x = 0 skipped, rounded once to float32.
float null2_correction(const float* null2, const uint8_t* codes, size_t Le);

// log(1 + omega exp(correction)), in float64, rounded once.
inline float null2_bias(double correction) {
    return static_cast<float>(std::log(1.0 + kNull2Omega * std::exp(correction)));
}
// (the null1 score, the bits and the tail are fwd_host.h's null1_score, bits_of and tail_pvalue: the pieces of
// fwd_pvalue_of, so "exactly as msv_fwd_pvalues computes it" is one text)

}  // namespace msv_host
