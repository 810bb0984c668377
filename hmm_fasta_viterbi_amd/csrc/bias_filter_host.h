// bias_filter_host.h -- host-only half of the bias filter (msv.h "Bias filter"): the two-state model of
// a profile's composition, its float64 Forward (the definition every test compares against), the filtered P-value
// arithmetic (shared with the device kernels of bias_filter.hip) and the builder of the device table.  No HIP
// include: bias_filter_host.cpp is built by plain g++ and runs under the sanitizers (tests/cpp/sanitize_bias.cpp).
#pragma once

#include <cstddef>
#include <cstdint>

#include "fwd_host.h"
#include "msv.h"

namespace msv_host {

// The model of msv.h's block in float64: state 0 emits the background (odds 1), state 1 the composition (odds r).
struct BfModel {
    double t00 = 0, t01 = 0, t10 = 0, t11 = 0;
    double pi0 = 0, pi1 = 0;
    double r[20] = {};
};
// compo, background: 20 floats each; model_length = LENG + 1 >= 2.  MSV_ERR_INVALID_ARGUMENT unless every compo
// value is finite and >= 0 and every background value finite and > 0.
msv_status bf_model(const float* compo, const float* background, uint32_t model_length, BfModel* out);
// bias(seq) in nats, 0 for L = 0; rescaled by exact powers of two.  *bad is set when a code >= 20 is met (the
// result is then meaningless).
double bf_score(const BfModel& m, const uint8_t* codes, size_t L, bool* bad);

// The device table: {t00, t01, t10, t11, pi0, pi1, r[0..19]} each rounded once from float64.  The kernel
// normalises a lane's product only after its 16 steps, so it needs 2^-24 <= r <= 2^7 for every residue (DESIGN
// 4.13; a composition and a background that are distributions give r <= 1 / min f < 88): MSV_ERR_UNSUPPORTED_MODEL
// otherwise.
constexpr int kBfTableFloats = 26;
constexpr int kBfTableT = 0, kBfTablePi = 4, kBfTableR = 6;
msv_status bf_device_table(const BfModel& m, float* table);

// The filtered P-values: msv_pvalue_of's and fwd_pvalue_of's arithmetic term for term, with the bias subtracted
// from the nats above null1 before they become bits.  x - 0.0f is x, so a zero bias gives their results bitwise.
FWD_HD inline double bf_gumbel_pvalue(float score, float bias, uint64_t L, float mu, float lambda) {
    if (L == 0) return 1.0;
    const float bits = bits_of(score - null1_score(L) - bias);
    const double y = static_cast<double>(lambda) * (static_cast<double>(bits) - static_cast<double>(mu));
    const double ey = -exp(-y);
    return fabs(ey) < 5e-9 ? -ey : 1.0 - exp(ey);
}
FWD_HD inline double bf_exponential_pvalue(float score, float bias, uint64_t L, float tau, float lambda) {
    if (L == 0) return 1.0;
    return tail_pvalue(bits_of(score - null1_score(L) - bias), tau, lambda);
}

}  // namespace msv_host
