// fwd_host.h -- host-only half of the Forward stage: the float64 CPU Forward every test compares
// against, the kernel-layout odds tables with the D-scan constants, and the P-value formula (shared with the
// device P-value kernel).  No HIP include: fwd_host.cpp is built by plain g++ and runs under the sanitizers
// (tests/cpp/sanitize_forward.cpp).
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "msv.h"

#if defined(__HIPCC__)
#define FWD_HD __host__ __device__
#else
#define FWD_HD
#endif

namespace msv_host {

// The three steps of a Forward P-value, each written once (the bias stage, null2_host.cpp, takes them apart to put
// its correction between the null1 score and the bits).  nullsc and bits are msv_pvalue_of's (float, as
// p7_bg_NullOne): the null1 score of a sequence of L >= 1 residues, the bit score of nats above it, and HMMER3's
// exponential tail over STATS LOCAL FORWARD.
FWD_HD inline float null1_score(uint64_t L) {
    const float p1 = static_cast<float>(L) / static_cast<float>(L + 1);
    return static_cast<float>(static_cast<double>(L) * log(static_cast<double>(p1)) +
                              log(1.0 - static_cast<double>(p1)));
}
FWD_HD inline float bits_of(float nats) { return nats / 0.69314718055994529f; }
FWD_HD inline double tail_pvalue(float bits, float tau, float lambda) {
    if (bits < tau) return 1.0;
    return exp(-static_cast<double>(lambda) * (static_cast<double>(bits) - static_cast<double>(tau)));
}
// Forward P-value of one score (msv.h, msv_fwd_pvalues); an empty sequence gives 1.
FWD_HD inline double fwd_pvalue_of(float score, uint64_t L, float tau, float lambda) {
    if (L == 0) return 1.0;
    return tail_pvalue(bits_of(score - null1_score(L)), tau, lambda);
}

// The model of msv.h's Forward block as float64 odds: x = exp((double)score), -inf -> 0.
struct FwdModel {
    size_t M = 0;                 // LENG + 1
    std::vector<double> xm, xi;   // [20][M] match / insert odds (xi = 1 without insert scores)
    std::vector<double> xt;       // [M][7] transition odds, nodes 1 .. LENG-1 (0 elsewhere)
    double tBM = 0, tEC = 0, tEJ = 0;
};
FwdModel fwd_model(const float* msc, const float* isc, const float* tsc, size_t M, float tr_B_Mk, float tr_E_C,
                   float tr_E_J);
// The serial float64 Forward of one sequence of codes 0..19, in nats (-inf for L = 0): rescaled odds, the
// scale a power of two, so the rescaling is exact.
double forward_run_on_sequence(const FwdModel& m, const uint8_t* codes, size_t L);

// Kernel-layout tables of a Forward variant of S states per lane (fwd_kernel.h): float32 odds, slot q of lane l
// is state k = l * S + q + 1, chunk c of a lane holds slots 2c, 2c + 1 as one float pair, lanes contiguous.
//   et, it : [20][S/2][64] pairs, match / insert odds (it empty unless isc); padding slots 0 (insert: 1, unused)
//   tt     : [8][S/2][64] pairs: the 7 per-slot transition arrays in vit_kernel.h's order, then the D-scan
//            prefix products c_q = tDD(slot 0) * .. * tDD(slot q) of the lane
//   scan   : [6][64] floats: step j's multiplier of lane l = the product of the lanes' whole-lane tDD products
//            c_{S-1} over lanes max(0, l - 2^j + 1) .. l
struct FwdTables {
    std::vector<float> et, it, tt, scan;
};
FwdTables fwd_tables(const float* msc, const float* isc_tab, const float* tsc, uint32_t model_length, int S, bool isc);

}  // namespace msv_host
