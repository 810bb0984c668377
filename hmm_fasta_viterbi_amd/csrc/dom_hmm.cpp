// dom_hmm.cpp -- Domain_HMM (msv_hmm.hpp) on the C-ABI of the domain stage.  The score tables are built exactly
// as Forward_HMM's (fwd_hmm.cpp), so the stages decode the model they scored.
#include <cmath>
#include <stdexcept>
#include <string>
#include <vector>

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

Domain_HMM::Domain_HMM(const Profile_HMM& base_hmm, int device, msv_insert_mode inserts)
    : model_length_(base_hmm.model_length), inserts_(inserts == MSV_INSERTS_LOG_ODDS) {
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
    check(msv_dom_profile_create(device, match_scores_.data(), inserts_ ? insert_scores_.data() : nullptr,
                                 transition_scores_.data(), static_cast<uint32_t>(M), tr_B_Mk_, tr_E_C_, tr_E_J_,
                                 &profile_),
          "msv_dom_profile_create");
}

Domain_HMM::~Domain_HMM() { msv_dom_profile_destroy(profile_); }

Decoded_sequence Domain_HMM::decode_on_sequence(const Protein_sequence& seq) {
    const size_t L = seq.empty() ? 0 : seq.size() - 1;
    std::vector<uint8_t> codes(L);
    if (L && msv_encode_residues(seq.data() + 1, L, codes.data()) != MSV_OK)
        throw std::out_of_range("residue outside the 20 amino acids");
    Decoded_sequence d;
    d.begin.resize(L);
    d.end.resize(L);
    d.occ.resize(L);
    check(msv_dom_cpu_decode(match_scores_.data(), inserts_ ? insert_scores_.data() : nullptr,
                             transition_scores_.data(), static_cast<uint32_t>(model_length_), tr_B_Mk_, tr_E_C_,
                             tr_E_J_, codes.data(), L, &d.forward_score, &d.backward_score, d.begin.data(),
                             d.end.data(), d.occ.data()),
          "msv_dom_cpu_decode");
    return d;
}

Envelopes Domain_HMM::decode_batch(const Packed_sequences& packed, const std::vector<uint32_t>& select, float rt1,
                                   float rt2, uint64_t workspace_bytes) {
    msv_dom_result* r = nullptr;
    const msv_status s =
        msv_dom_decode_batch(profile_, packed.codes.data(), packed.offsets.data(), packed.size(),
                             select.empty() ? nullptr : select.data(), select.size(), rt1, rt2, workspace_bytes, &r);
    if (s == MSV_ERR_BAD_RESIDUE) {
        msv_dom_result_free(r);
        throw std::out_of_range("residue outside the 20 amino acids");
    }
    if (s != MSV_OK) msv_dom_result_free(r);
    check(s, "msv_dom_decode_batch");
    Envelopes e;
    const uint64_t m = msv_dom_result_count(r);
    e.forward_scores.resize(m);
    e.backward_scores.resize(m);
    e.residue_offsets.resize(m + 1);
    e.region_offsets.resize(m + 1);
    e.begin.resize(msv_dom_result_residues(r));
    e.end.resize(e.begin.size());
    e.occ.resize(e.begin.size());
    e.regions.resize(msv_dom_result_regions(r));
    const msv_status c =
        msv_dom_result_copy(r, e.forward_scores.data(), e.backward_scores.data(), e.residue_offsets.data(),
                            e.begin.data(), e.end.data(), e.occ.data(), e.region_offsets.data(), e.regions.data());
    msv_dom_result_free(r);
    check(c, "msv_dom_result_copy");
    return e;
}

Split_regions Domain_HMM::split_regions(const Packed_sequences& packed, const Envelopes& e, float rt3,
                                        uint32_t n_samples, uint64_t seed, uint64_t workspace_bytes) {
    Split_regions out;
    const size_t n_regions = e.regions.size();
    out.multidomain.assign(n_regions, 0);
    std::vector<msv_aln_item> multi;
    for (size_t q = 0; q + 1 < e.region_offsets.size(); ++q) {
        const uint64_t r0 = e.residue_offsets[q], L = e.residue_offsets[q + 1] - r0;
        for (uint64_t g = e.region_offsets[q]; g < e.region_offsets[q + 1]; ++g) {
            const msv_dom_region& r = e.regions[g];
            int is_multi = 0;
            check(msv_dom_is_multidomain(e.begin.data() + r0, e.end.data() + r0, L, r.i_from, r.i_to, rt3, &is_multi),
                  "msv_dom_is_multidomain");
            out.multidomain[g] = static_cast<uint8_t>(is_multi);
            if (is_multi) multi.push_back(msv_aln_item{r.seq, r.i_from, r.i_to});
        }
    }
    msv_spl_options opt{};
    opt.struct_size = sizeof(opt);
    opt.workspace_bytes = workspace_bytes;
    opt.seed = seed;
    opt.seed_set = 1;
    opt.n_samples = n_samples;
    msv_spl_result* r = nullptr;
    const msv_status s = msv_spl_sample_batch(profile_, packed.codes.data(), packed.offsets.data(), packed.size(),
                                              multi.data(), multi.size(), &opt, &r);
    if (s == MSV_ERR_BAD_RESIDUE) {
        msv_spl_result_free(r);
        throw std::out_of_range("residue outside the 20 amino acids");
    }
    if (s != MSV_OK) msv_spl_result_free(r);
    check(s, "msv_spl_sample_batch");
    msv_spl_stats stats{};
    stats.struct_size = sizeof(stats);
    msv_status c = msv_spl_result_stats(r, &stats);
    std::vector<msv_spl_segment> segs(msv_spl_result_segments(r));
    std::vector<uint64_t> off(multi.size() * static_cast<size_t>(stats.n_samples) + 1, 0);
    if (c == MSV_OK) c = msv_spl_result_copy(r, nullptr, off.data(), segs.data());
    msv_spl_result_free(r);
    check(c, "msv_spl_result_copy");
    out.truncated = stats.truncated;
    size_t at = 0;  // the next multi-domain region's place in `multi`
    for (size_t g = 0; g < n_regions; ++g) {
        const msv_dom_region& reg = e.regions[g];
        if (!out.multidomain[g]) {
            out.items.push_back(msv_aln_item{reg.seq, reg.i_from, reg.i_to});
            out.region.push_back(g);
            out.prob.push_back(1.0f);
            continue;
        }
        const uint64_t lo = off[at * stats.n_samples], hi = off[(at + 1) * stats.n_samples];
        ++at;
        uint32_t n_env = 0;
        check(msv_spl_cluster(segs.data() + lo, hi - lo, stats.n_samples, nullptr, &n_env, nullptr), "msv_spl_cluster");
        std::vector<msv_spl_envelope> env(n_env);
        if (n_env)
            check(msv_spl_cluster(segs.data() + lo, hi - lo, stats.n_samples, nullptr, &n_env, env.data()),
                  "msv_spl_cluster");
        for (const msv_spl_envelope& c2 : env) {
            out.items.push_back(msv_aln_item{reg.seq, c2.i_from, c2.i_to});
            out.region.push_back(g);
            out.prob.push_back(c2.prob);
        }
    }
    return out;
}
