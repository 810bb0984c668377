// fwd_hmm.cpp -- Forward_HMM and search_pipeline (msv_hmm.hpp) on the C-ABI of the Forward stage.  The score
// tables are built exactly as Viterbi_HMM's (msv_hmm.cpp), so the three stages score one model.
#include <cmath>
#include <stdexcept>
#include <string>
#include <vector>

#include "fwd_host.h"
#include "msv.h"
#include "msv_hmm.hpp"

namespace {

void check(msv_status s, const char* what) {
    if (s != MSV_OK) throw msv_error(s, std::string(what) + ": " + msv_status_string(s));
}

// background_frequencies, MSV_HMM.cpp:21-27 (msv_hmm.cpp's table)
constexpr float kBackground[NUM_OF_AMINO_ACIDS] = {
    0.0787945f, 0.0151600f, 0.0535222f, 0.0668298f, 0.0397062f, 0.0695071f, 0.0229198f,
    0.0590092f, 0.0594422f, 0.0963728f, 0.0237718f, 0.0414386f, 0.0482904f, 0.0395639f,
    0.0540978f, 0.0683364f, 0.0540687f, 0.0673417f, 0.0114135f, 0.0304133f};

}  // namespace

Forward_HMM::Forward_HMM(const Profile_HMM& base_hmm, int device, msv_insert_mode inserts)
    : forward_tau(base_hmm.stats_local_forward_theta),
      forward_lambda(base_hmm.stats_local_forward_lambda),
      model_length_(base_hmm.model_length),
      inserts_(inserts == MSV_INSERTS_LOG_ODDS) {
    const size_t M = model_length_;
    match_scores_.assign(NUM_OF_AMINO_ACIDS * M, 0.f);
    insert_scores_.assign(NUM_OF_AMINO_ACIDS * M, 0.f);
    transition_scores_.assign(NUM_OF_TRANSITIONS * M, 0.f);
    for (size_t k = 0; k < M; ++k) {
        for (size_t r = 0; r < NUM_OF_AMINO_ACIDS; ++r) {
            match_scores_[r * M + k] = std::log(base_hmm.match_emissions[k][r] / kBackground[r]);
            if (inserts_) insert_scores_[r * M + k] = std::log(base_hmm.insert_emissions[k][r] / kBackground[r]);
        }
        for (size_t t = 0; t < NUM_OF_TRANSITIONS; ++t)
            transition_scores_[k * NUM_OF_TRANSITIONS + t] = std::log(base_hmm.transitions[k][t]);
    }
    constexpr float nu = 2.0;  // the MSV path's specials, MSV_HMM.cpp:49-53
    tr_B_Mk_ = std::log(2.0f / static_cast<float>(M * (M + 1)));
    tr_E_C_ = std::log((nu - 1.0f) / nu);
    tr_E_J_ = std::log(1.0f / nu);
    check(msv_fwd_profile_create(device, match_scores_.data(), inserts_ ? insert_scores_.data() : nullptr,
                                 transition_scores_.data(), static_cast<uint32_t>(M), tr_B_Mk_, tr_E_C_, tr_E_J_,
                                 &profile_),
          "msv_fwd_profile_create");
}

Forward_HMM::~Forward_HMM() { msv_fwd_profile_destroy(profile_); }

double Forward_HMM::run_on_sequence(const Protein_sequence& seq) {
    const size_t L = seq.empty() ? 0 : seq.size() - 1;
    std::vector<uint8_t> codes(L);
    if (L && msv_encode_residues(seq.data() + 1, L, codes.data()) != MSV_OK)
        throw std::out_of_range("residue outside the 20 amino acids");
    const msv_host::FwdModel m =
        msv_host::fwd_model(match_scores_.data(), inserts_ ? insert_scores_.data() : nullptr,
                            transition_scores_.data(), model_length_, tr_B_Mk_, tr_E_C_, tr_E_J_);
    return msv_host::forward_run_on_sequence(m, codes.data(), L);
}

Log_score Forward_HMM::parallel_run_on_sequence(const Protein_sequence& seq) {
    return score_batch(Protein_sequences{seq})[0];
}

std::vector<Log_score> Forward_HMM::score_batch(const Protein_sequences& seqs) {
    return score_batch(Packed_sequences::pack(seqs));
}

std::vector<Log_score> Forward_HMM::score_batch(const Packed_sequences& packed) {
    std::vector<Log_score> out(packed.size());
    const msv_status s = msv_fwd_score_batch(profile_, packed.codes.data(), packed.offsets.data(), packed.size(),
                                             out.data(), nullptr);
    if (s == MSV_ERR_BAD_RESIDUE) throw std::out_of_range("residue outside the 20 amino acids");
    check(s, "msv_fwd_score_batch");
    return out;
}

std::vector<double> Forward_HMM::pvalues(const std::vector<Log_score>& scores, const Packed_sequences& packed) const {
    if (scores.size() != packed.size()) throw msv_error(MSV_ERR_INVALID_ARGUMENT, "scores and sequences disagree");
    std::vector<double> out(scores.size());
    check(msv_fwd_pvalues(scores.data(), packed.offsets.data(), scores.size(), forward_tau, forward_lambda, out.data()),
          "msv_fwd_pvalues");
    return out;
}

Search_result search_pipeline(MSV_HMM& msv, Viterbi_HMM& vit, Forward_HMM& fwd, const Packed_sequences& packed,
                              const Profile_HMM& stats, double F1, double F2) {
    const size_t n = packed.size();
    Search_result r;
    r.msv_scores.resize(n);
    r.viterbi_scores.resize(n);
    r.forward_scores.resize(n);
    r.passed_msv.resize(n);
    r.passed_viterbi.resize(n);
    r.forward_pvalues.resize(n);
    const float st[6] = {stats.stats_local_msv_mu,        stats.stats_local_msv_lambda,
                         stats.stats_local_viterbi_mu,    stats.stats_local_viterbi_lambda,
                         stats.stats_local_forward_theta, stats.stats_local_forward_lambda};
    uint64_t n1 = 0, n2 = 0;
    const msv_status s = msv_fwd_filter_batch(
        msv.handle(), vit.handle(), fwd.handle(), packed.codes.data(), packed.offsets.data(), n, st, F1, F2,
        r.msv_scores.data(), r.passed_msv.data(), r.viterbi_scores.data(), r.passed_viterbi.data(),
        r.forward_scores.data(), r.forward_pvalues.data(), &n1, &n2);
    if (s == MSV_ERR_BAD_RESIDUE) throw std::out_of_range("residue outside the 20 amino acids");
    check(s, "msv_fwd_filter_batch");
    r.n_passed_msv = n1;
    r.n_passed_viterbi = n2;
    return r;
}
