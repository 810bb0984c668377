// null2_host.cpp -- the bias stage on the host (msv.h "Bias stage" states the model): the float64 null2
// of an envelope by expectation, the definition of the correction, the bias / bit score / P-value arithmetic.  Host
// only, no HIP.
#include "null2_host.h"

#include <cmath>
#include <limits>
#include <vector>

#include "aln_host.h"

namespace msv_host {

namespace {
// the float32 odds the device tables hold (fwd_tables), as float64
inline double odds32(float score) { return static_cast<double>(static_cast<float>(std::exp(static_cast<double>(score)))); }
}  // namespace

void null2_on_envelope(const FwdModel& m, const float* msc, const float* isc, const uint8_t* codes, size_t Le, size_t Lc,
                       double* null2, double* domcorrection) {
    const size_t M = m.M, K = M - 1;
    std::vector<double> pm(Le * M, 0.0), pi(Le * M, 0.0), pn(Le, 0.0), pj(Le, 0.0), pc(Le, 0.0);
    aln_decode_on_envelope(m, codes, Le, Lc, nullptr, pm.data(), pi.data(), pn.data(), pj.data(), pc.data());
    std::vector<double> eM(M, 0.0), eI(M, 0.0);
    double eX = 0.0;
    for (size_t i = 0; i < Le; ++i) {
        for (size_t k = 1; k <= K; ++k) eM[k] += pm[i * M + k];
        for (size_t k = 1; k < K; ++k) eI[k] += pi[i * M + k];
        eX += pn[i] + pj[i] + pc[i];
    }
    double n2[kNull2Residues];
    for (size_t x = 0; x < kNull2Residues; ++x) {
        double t = 0.0;
        for (size_t k = 1; k <= K; ++k) t += eM[k] * odds32(msc[x * M + k]);
        for (size_t k = 1; k < K; ++k) t += eI[k] * (isc ? odds32(isc[x * M + k]) : 1.0);
        n2[x] = (t + eX) / static_cast<double>(Le);
        if (null2) null2[x] = n2[x];
    }
    if (domcorrection) {
        uint64_t count[kNull2Residues] = {};
        for (size_t i = 0; i < Le; ++i) count[codes[i]] += 1;
        double dc = 0.0;
        for (size_t x = 0; x < kNull2Residues; ++x)
            if (count[x]) dc += static_cast<double>(count[x]) * std::log(n2[x]);
        *domcorrection = dc;
    }
}

float null2_correction(const float* null2, const uint8_t* codes, size_t Le) {
    uint64_t count[kNull2Residues] = {};
    for (size_t i = 0; i < Le; ++i)
        if (codes[i] < kNull2Residues) count[codes[i]] += 1;
    double dc = 0.0;
    for (size_t x = 0; x < kNull2Residues; ++x)
        if (count[x]) dc += static_cast<double>(count[x]) * std::log(static_cast<double>(null2[x]));
    return static_cast<float>(dc);
}

}  // namespace msv_host

extern "C" {

msv_status msv_aln_cpu_null2(const float* match_scores, const float* insert_scores, const float* transition_scores,
                             uint32_t model_length, float tr_B_Mk, float tr_E_C, float tr_E_J, const uint8_t* codes,
                             uint64_t Le, uint64_t Lc, double* null2, double* domcorrection) {
    if (!match_scores || !transition_scores || model_length < 2 || !codes || Le == 0 || Lc < Le || Lc >= (1ull << 31))
        return MSV_ERR_INVALID_ARGUMENT;
    for (uint64_t i = 0; i < Le; ++i)
        if (codes[i] >= 20) return MSV_ERR_BAD_RESIDUE;
    const msv_host::FwdModel m = msv_host::fwd_model(match_scores, insert_scores, transition_scores, model_length,
                                                     tr_B_Mk, tr_E_C, tr_E_J);
    msv_host::null2_on_envelope(m, match_scores, insert_scores, codes, Le, Lc, null2, domcorrection);
    return MSV_OK;
}

msv_status msv_aln_null2_correction(const float* null2, const uint8_t* codes, uint64_t Le, float* domcorrection) {
    if (!null2 || !domcorrection || (Le && !codes)) return MSV_ERR_INVALID_ARGUMENT;
    for (uint64_t i = 0; i < Le; ++i)
        if (codes[i] >= 20) return MSV_ERR_BAD_RESIDUE;
    *domcorrection = msv_host::null2_correction(null2, codes, Le);
    return MSV_OK;
}

msv_status msv_aln_bias_scores(const float* envelope_scores, const uint64_t* Le, const uint64_t* Lc,
                               const float* domcorrection, uint64_t m, const uint32_t* parent, const float* fwd_scores,
                               const uint64_t* seq_lengths, uint64_t n_seq, float tau, float lambda, float* dombias,
                               float* domain_bits, double* domain_pvalues, float* seq_bias, float* seq_bits,
                               double* seq_pvalues) {
    if (m && (!envelope_scores || !Le || !Lc || !domcorrection)) return MSV_ERR_INVALID_ARGUMENT;
    if (n_seq && (!fwd_scores || !seq_lengths || (m && !parent))) return MSV_ERR_INVALID_ARGUMENT;
    for (uint64_t q = 0; q < m; ++q) {
        if (Le[q] == 0 || Lc[q] < Le[q] || Lc[q] >= (1ull << 31)) return MSV_ERR_INVALID_ARGUMENT;
        if (n_seq && parent[q] >= n_seq) return MSV_ERR_INVALID_ARGUMENT;
    }
    for (uint64_t q = 0; q < m; ++q) {
        float loop, move;
        msv_sequence_transitions(Lc[q], &loop, &move);
        const float bias = msv_host::null2_bias(static_cast<double>(domcorrection[q]));
        // HMMER's per-domain score: the envelope score plus the flanks emitted by N / C, float adds on float values
        const float flank = (static_cast<float>(Lc[q]) - static_cast<float>(Le[q])) * loop;
        const float domsc = envelope_scores[q] + flank;
        const float bits = msv_host::bits_of(domsc - msv_host::null1_score(Lc[q]) - bias);
        if (dombias) dombias[q] = bias;
        if (domain_bits) domain_bits[q] = bits;
        if (domain_pvalues) domain_pvalues[q] = msv_host::tail_pvalue(bits, tau, lambda);
    }
    if (n_seq) {
        std::vector<double> sum(n_seq, 0.0);
        for (uint64_t q = 0; q < m; ++q) sum[parent[q]] += static_cast<double>(domcorrection[q]);
        for (uint64_t s = 0; s < n_seq; ++s) {
            const float bias = msv_host::null2_bias(sum[s]);
            const bool empty = seq_lengths[s] == 0;
            const float bits = empty ? -std::numeric_limits<float>::infinity()
                                     : msv_host::bits_of(fwd_scores[s] - msv_host::null1_score(seq_lengths[s]) - bias);
            if (seq_bias) seq_bias[s] = bias;
            if (seq_bits) seq_bits[s] = bits;
            if (seq_pvalues) seq_pvalues[s] = empty ? 1.0 : msv_host::tail_pvalue(bits, tau, lambda);
        }
    }
    return MSV_OK;
}

}  // extern "C"
