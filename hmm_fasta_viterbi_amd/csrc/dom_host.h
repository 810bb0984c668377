// dom_host.h -- host-only half of the domain stage: the float64 CPU Forward / Backward decode every
// test compares against, the envelope rule (shared, as one inline function, with the device kernel), the
// kernel-layout Backward tables with the mirrored D-scan constants, and the workspace arithmetic.  No HIP include:
// dom_host.cpp is built by plain g++ and runs under the sanitizers (tests/cpp/sanitize_decode.cpp).
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "fwd_host.h"
#include "msv.h"

namespace msv_host {

// One float64 decode of a sequence of codes 0..19 (msv.h, "Domain stage"): both scores in nats and, when the
// pointers are given, begin / end / occ as double [L].  L = 0: both scores -inf, nothing written.
void decode_run_on_sequence(const FwdModel& m, const uint8_t* codes, size_t L, double* fwd_score, double* bck_score,
                            double* begin, double* end, double* occ);

// The envelope rule of msv.h on three float arrays of one sequence (residue i at index i - 1).  emit(i_from, i_to,
// expected_domains, mass) is called once per region, in order; returns the number of regions.  The ONE definition
// of the rule: msv_dom_regions and both device kernels (dom_kernel.hip) are this function.  The differences are
// plain float subtractions and the sums plain float additions.  The function holds no multiply, so there is nothing
// a compiler could contract into an FMA: the host object (plain g++ flags, no -ffp-contract=off) and the device
// object (built with it) round alike.
template <class Emit>
FWD_HD inline uint32_t dom_regions_scan(const float* begin, const float* end, const float* occ, uint64_t L, float rt1,
                                        float rt2, Emit emit) {
    uint32_t n = 0;
    uint64_t start = 0;  // 0: unset
    bool triggered = false;
    for (uint64_t j = 1; j <= L; ++j) {
        const float o = occ[j - 1];
        if (!triggered) {
            const float d = o - begin[j - 1];
            if (d < rt2) start = j;
            else if (start == 0) start = j;
            if (o >= rt1) triggered = true;
        } else {
            const float d = o - end[j - 1];
            if (d < rt2) {
                float nd = 0.0f, mass = 0.0f;
                for (uint64_t i = start; i <= j; ++i) {
                    nd = nd + begin[i - 1];
                    mass = mass + occ[i - 1];
                }
                emit(static_cast<uint32_t>(start), static_cast<uint32_t>(j), nd, mass);
                ++n;
                start = 0;
                triggered = false;
            }
        }
    }
    return n;
}

// Kernel-layout tables of a domain-stage variant of S states per lane (dom_kernel.h).  The recording Forward
// kernel reads fwd_tables' et / it / tt / scan unchanged; the Backward kernel reads et / it and
//   bt    : [8][S/2][64] pairs: the 7 per-slot transition arrays indexed by the slot's OWN node k (m->m, m->i, m->d,
//           i->m, i->i, d->m, d->d of node k: 0 at k >= LENG and in padding slots), then the D-scan suffix
//           products s_q = tDD(slot q) * .. * tDD(slot S-1) of the lane
//   bscan : [6][64] floats: step j's multiplier of lane l = the product of the lanes' whole-lane products s_0 over
//           lanes l .. min(63, l + 2^j - 1)
struct DomTables {
    FwdTables fwd;
    std::vector<float> bt, bscan;
};
DomTables dom_tables(const float* msc, const float* isc_tab, const float* tsc, uint32_t model_length, int S, bool isc);

// Workspace of one selected sequence of L residues: the recording kernel's L + 1 rows (row 0 included) of six
// 32-bit words {N, J, C, B, E, exponent}.
constexpr uint64_t kDomRowWords = 6;
inline uint64_t dom_sequence_bytes(uint64_t L) { return (L + 1) * kDomRowWords * sizeof(uint32_t); }

}  // namespace msv_host
