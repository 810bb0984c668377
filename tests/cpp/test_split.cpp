// test_split.cpp -- the C++ Domain_HMM::split_regions (msv_hmm.hpp, csrc/dom_hmm.cpp) on a profile and a FASTA file
// given by the caller: decode_batch, then split_regions with its defaults.  Every unsplit region must be its own item
// with prob 1, every item of a multi-domain region must lie inside that region, and the multi-domain flags must be
// msv_dom_is_multidomain's on the returned arrays.  The items are printed, one a line, for the caller to compare
// (tests/test_gpu_split.py compares them with the Python surface's).
// Usage: test_split <profile.hmm> <sequences.fsa>   (exit 0 = pass)
#include <cstdio>
#include <string>
#include <vector>

#include "msv_hmm.hpp"

#define REQUIRE(cond)                                                            \
    do {                                                                         \
        if (!(cond)) {                                                           \
            std::printf("test_split failed! %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            return 1;                                                            \
        }                                                                        \
    } while (0)

int main(int argc, char** argv) {
    if (argc < 3) {
        std::printf("usage: test_split <profile.hmm> <sequences.fsa>\n");
        return 2;
    }
    const Profile_HMM prof(argv[1]);
    auto fasta = FASTA_protein_sequences(argv[2]);
    Domain_HMM dom(prof);
    const Packed_sequences packed = Packed_sequences::pack(fasta.sequences);
    const Envelopes env = dom.decode_batch(packed);
    const Split_regions split = dom.split_regions(packed, env);
    REQUIRE(split.multidomain.size() == env.regions.size());
    REQUIRE(split.items.size() == split.region.size() && split.items.size() == split.prob.size());
    REQUIRE(split.truncated == 0);
    size_t g = 0;
    for (size_t q = 0; q + 1 < env.region_offsets.size(); ++q) {
        const uint64_t r0 = env.residue_offsets[q], L = env.residue_offsets[q + 1] - r0;
        for (; g < env.region_offsets[q + 1]; ++g) {
            int multi = -1;
            REQUIRE(msv_dom_is_multidomain(env.begin.data() + r0, env.end.data() + r0, L, env.regions[g].i_from,
                                           env.regions[g].i_to, 0.20f, &multi) == MSV_OK);
            REQUIRE(multi == split.multidomain[g]);
        }
    }
    uint64_t prev = 0;
    for (size_t j = 0; j < split.items.size(); ++j) {
        const msv_aln_item& it = split.items[j];
        REQUIRE(split.region[j] >= prev && split.region[j] < env.regions.size());
        prev = split.region[j];
        const msv_dom_region& r = env.regions[split.region[j]];
        REQUIRE(it.seq == r.seq && it.i_from >= r.i_from && it.i_to <= r.i_to && it.i_from <= it.i_to);
        if (!split.multidomain[split.region[j]])
            REQUIRE(it.i_from == r.i_from && it.i_to == r.i_to && split.prob[j] == 1.0f);
        else
            REQUIRE(split.prob[j] >= 0.25f && split.prob[j] <= 1.0f);
        std::printf("item %u %u %u region %llu prob %.9g\n", it.seq, it.i_from, it.i_to,
                    static_cast<unsigned long long>(split.region[j]), static_cast<double>(split.prob[j]));
    }
    std::printf("test_split passed: %zu regions, %zu items\n", env.regions.size(), split.items.size());
    return 0;
}
