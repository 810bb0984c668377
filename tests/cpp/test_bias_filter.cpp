// test_bias_filter.cpp -- the C++ Bias_filter surface (msv_hmm.hpp) on 100.hmm x the sequences of data/FASTA_files:
// score_batch (GPU) against run_on_sequence (the float64 definition) at msv.h's tolerance, a batch of one, the
// filtered P-values with a zero bias against msv_pvalues, and the error path (a residue outside the 20 throws
// std::out_of_range, as Forward_HMM::score_batch does).
// Usage: test_bias_filter <repo_root>   (exit 0 = pass)
#include <cmath>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "msv_hmm.hpp"

#define REQUIRE(cond)                                                                       \
    do {                                                                                    \
        if (!(cond)) {                                                                      \
            std::printf("test_bias_filter failed! %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            return 1;                                                                       \
        }                                                                                   \
    } while (0)

static double tolerance(double L, double cpu) {
    const double u = 0x1p-24, k = 5.0 * L + 14.0 * std::ceil(L / 1024.0) + 4.0;
    return k * u / (1.0 - k * u) + u * std::fabs(cpu);
}

int main(int argc, char** argv) {
    const std::string root = argc > 1 ? argv[1] : ".";
    const std::string path = root + "/data/profile_HMMs/100.hmm";
    const Profile_HMM prof(path);
    // Profile_HMM keeps the reference's members only (a caller built against an earlier header allocates exactly
    // these); the COMPO line is read apart
    REQUIRE(sizeof(Profile_HMM) ==
            sizeof(Profile_name) + 3 * sizeof(std::vector<float>) + sizeof(size_t) + 6 * sizeof(float));
    Bias_filter bf(path);
    REQUIRE(bf.model_length() == prof.model_length && bf.handle() != nullptr);
    double total = 0;
    for (float c : bf.compo()) total += c;
    REQUIRE(std::fabs(total - 1.0) < 1e-5);
    {
        Bias_filter same(prof, profile_compo(path));  // the form over an already parsed profile
        REQUIRE(same.compo() == bf.compo() && same.model_length() == bf.model_length());
    }
    size_t scored = 0;
    for (const char* name : {"fasta_like_example.fsa", "random_FASTA.fsa"}) {
        FASTA_protein_sequences* fasta = new FASTA_protein_sequences(root + "/data/FASTA_files/" + name);
        const Packed_sequences& packed = fasta->packed;
        const std::vector<Log_score> got = bf.score_batch(packed);
        REQUIRE(got.size() == packed.size());
        for (size_t s = 0; s < packed.size(); ++s) {
            const double want = bf.run_on_sequence(fasta->sequences[s]);
            const double L = static_cast<double>(packed.offsets[s + 1] - packed.offsets[s]);
            REQUIRE(std::fabs(got[s] - want) <= tolerance(L, want));
            ++scored;
        }
        if (packed.size()) {
            const Log_score one = bf.parallel_run_on_sequence(fasta->sequences[0]);
            REQUIRE(std::memcmp(&one, &got[0], sizeof(float)) == 0);  // a bias does not depend on the batch
            // a zero bias gives msv_pvalues' values
            const std::vector<Log_score> zero(packed.size(), 0.0f);
            const std::vector<double> pv = bf.pvalues(got, zero, packed, prof.stats_local_msv_mu,
                                                      prof.stats_local_msv_lambda, MSV_BF_GUMBEL);
            std::vector<double> ref(packed.size());
            REQUIRE(msv_pvalues(got.data(), packed.offsets.data(), packed.size(), prof.stats_local_msv_mu,
                                prof.stats_local_msv_lambda, ref.data()) == MSV_OK);
            REQUIRE(std::memcmp(pv.data(), ref.data(), pv.size() * sizeof(double)) == 0);
        }
        delete fasta;
    }
    REQUIRE(scored >= 2);
    // a residue outside the 20: the packer refuses the letter, the kernel the code
    bool threw = false;
    try {
        (void)bf.score_batch(Protein_sequences{"#ACDX"});
    } catch (const std::out_of_range&) {
        threw = true;
    }
    REQUIRE(threw);
    Packed_sequences bad;
    bad.codes = {0, 1, 2, 20};
    bad.offsets = {0, 4};
    threw = false;
    try {
        (void)bf.score_batch(bad);
    } catch (const std::out_of_range&) {
        threw = true;
    }
    REQUIRE(threw);
    std::printf("test_bias_filter passed: %zu sequences within tolerance\n", scored);
    return 0;
}
