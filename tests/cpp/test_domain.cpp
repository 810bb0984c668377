// test_domain.cpp -- the C++ Domain_HMM surface (msv_hmm.hpp, csrc/dom_hmm.cpp) on 100.hmm x
// fasta_like_example.fsa: decode_batch (GPU) against decode_on_sequence (the float64 CPU twin) at msv.h's
// tolerances, the regions against msv_dom_regions on the returned arrays, a select list, and the error path (a
// residue outside the 20 throws std::out_of_range, as Forward_HMM::score_batch does).
// Usage: test_domain <repo_root>   (exit 0 = pass)
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "msv_hmm.hpp"

#define REQUIRE(cond)                                                             \
    do {                                                                          \
        if (!(cond)) {                                                            \
            std::printf("test_domain failed! %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            return 1;                                                             \
        }                                                                         \
    } while (0)

int main(int argc, char** argv) {
    const std::string root = argc > 1 ? argv[1] : ".";
    const Profile_HMM prof(root + "/data/profile_HMMs/100.hmm");
    auto fasta = FASTA_protein_sequences(root + "/data/FASTA_files/fasta_like_example.fsa");
    Domain_HMM dom(prof);
    Forward_HMM fwd(prof);
    REQUIRE(dom.model_length() == prof.model_length && dom.handle() != nullptr);
    const Packed_sequences packed = Packed_sequences::pack(fasta.sequences);
    const size_t n = packed.size();
    REQUIRE(n >= 2);
    const double leng = static_cast<double>(prof.model_length - 1);
    const Envelopes all = dom.decode_batch(packed);
    REQUIRE(all.forward_scores.size() == n && all.residue_offsets.size() == n + 1 && all.region_offsets.size() == n + 1);
    REQUIRE(all.region_offsets[n] == all.regions.size() && all.residue_offsets[n] == all.begin.size());
    const std::vector<Log_score> fscores = fwd.score_batch(packed);
    size_t residues = 0;
    for (size_t s = 0; s < n; ++s) {
        const Decoded_sequence ref = dom.decode_on_sequence(fasta.sequences[s]);
        const size_t L = ref.begin.size(), o = all.residue_offsets[s];
        REQUIRE(all.residue_offsets[s + 1] - o == L);
        REQUIRE(std::memcmp(&all.forward_scores[s], &fscores[s], sizeof(float)) == 0);  // the Forward kernel's bits
        const double stol = 16.0 * (L + leng) * 0x1p-24 + 4.0 * 0x1p-24 * std::fabs(ref.forward_score);
        REQUIRE(std::fabs(all.forward_scores[s] - ref.forward_score) <= stol);
        REQUIRE(std::fabs(all.backward_scores[s] - ref.forward_score) <= stol);
        const double tol = 48.0 * (L + leng) * 0x1p-24 + 8.0 * 0x1p-24;
        for (size_t i = 0; i < L; ++i) {
            REQUIRE(std::fabs(all.begin[o + i] - ref.begin[i]) <= tol);
            REQUIRE(std::fabs(all.end[o + i] - ref.end[i]) <= tol);
            REQUIRE(std::fabs(all.occ[o + i] - ref.occ[i]) <= tol);
        }
        // the regions are the rule on the returned arrays
        uint32_t count = 0;
        REQUIRE(msv_dom_regions(all.begin.data() + o, all.end.data() + o, all.occ.data() + o, L, 0.25f, 0.10f, &count,
                                nullptr) == MSV_OK);
        REQUIRE(count == all.region_offsets[s + 1] - all.region_offsets[s]);
        std::vector<msv_dom_region> want(count);
        REQUIRE(msv_dom_regions(all.begin.data() + o, all.end.data() + o, all.occ.data() + o, L, 0.25f, 0.10f, &count,
                                want.data()) == MSV_OK);
        for (uint32_t r = 0; r < count; ++r) {
            const msv_dom_region& got = all.regions[all.region_offsets[s] + r];
            REQUIRE(got.seq == s && got.i_from == want[r].i_from && got.i_to == want[r].i_to);
            REQUIRE(got.expected_domains == want[r].expected_domains && got.mass == want[r].mass);
        }
        residues += L;
    }
    // a select list, in the caller's order, through a workspace that holds one sequence at a time
    uint64_t longest = 0;
    for (size_t s = 0; s < n; ++s) longest = std::max<uint64_t>(longest, all.residue_offsets[s + 1] - all.residue_offsets[s]);
    const std::vector<uint32_t> select = {static_cast<uint32_t>(n - 1), 0};
    const Envelopes two = dom.decode_batch(packed, select, 0.25f, 0.10f, msv_dom_sequence_bytes(longest));
    REQUIRE(two.forward_scores.size() == 2);
    for (size_t q = 0; q < 2; ++q) {
        const size_t s = select[q], L = two.residue_offsets[q + 1] - two.residue_offsets[q];
        REQUIRE(L == all.residue_offsets[s + 1] - all.residue_offsets[s]);
        REQUIRE(std::memcmp(&two.backward_scores[q], &all.backward_scores[s], sizeof(float)) == 0);
        REQUIRE(std::memcmp(two.occ.data() + two.residue_offsets[q], all.occ.data() + all.residue_offsets[s],
                            L * sizeof(float)) == 0);
    }
    // a residue outside the 20
    Packed_sequences bad = packed;
    bad.codes[3] = 20;
    bool thrown = false;
    try {
        (void)dom.decode_batch(bad);
    } catch (const std::out_of_range&) {
        thrown = true;
    }
    REQUIRE(thrown);
    const Envelopes again = dom.decode_batch(packed);  // the profile is usable afterwards, its error word cleared
    REQUIRE(std::memcmp(again.occ.data(), all.occ.data(), all.occ.size() * sizeof(float)) == 0);
    std::printf("test_domain passed: %zu sequences, %zu residues, %zu regions\n", n, residues, all.regions.size());
    return 0;
}
