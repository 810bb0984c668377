// sanitize_trace.cpp -- the Viterbi trace's host half under AddressSanitizer / UBSan (csrc/Makefile `asan_trace`):
// the CPU trace (msv_vit_cpu_trace) on tiny random models and on bundled profiles, the chunk cuts and the
// back-pointer layout, on the cases of tests/test_viterbi_trace_host.py.  Host-only sources, its own main.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <string>
#include <vector>

#include "msv.h"

#define REQUIRE(cond)                                                        \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                    \
        }                                                                    \
    } while (0)

namespace {

struct Tables {
    std::vector<float> msc, isc, tsc;
    uint32_t M = 0;
    float b = 0, c = 0, j = 0;
    bool inserts = false;
};

uint32_t bits(float x) {
    uint32_t u;
    static_assert(sizeof(u) == sizeof(x), "float32");
    std::memcpy(&u, &x, sizeof(u));
    return u;
}

// Traces one sequence by the two-call protocol and checks the path: legal, consistent, score == the score call's.
uint32_t trace_and_check(const Tables& t, const std::vector<uint8_t>& codes) {
    const float* isc = t.inserts ? t.isc.data() : nullptr;
    const uint8_t* cp = codes.empty() ? nullptr : codes.data();
    float sc = 0, want = 0;
    uint32_t nd = 0;
    uint64_t no = 0;
    REQUIRE(msv_vit_cpu_trace(t.msc.data(), isc, t.tsc.data(), t.M, t.b, t.c, t.j, cp, codes.size(), &sc, &nd, &no,
                              nullptr, nullptr) == MSV_OK);
    REQUIRE(msv_vit_cpu_score(t.msc.data(), isc, t.tsc.data(), t.M, t.b, t.c, t.j, cp, codes.size(), &want) == MSV_OK);
    REQUIRE(bits(sc) == bits(want));
    // exactly sized buffers: a write past either end is the sanitizer's to find
    std::vector<msv_vit_domain> doms(nd);
    std::vector<uint8_t> ops(no);
    msv_vit_domain dummy_d;
    uint8_t dummy_o;
    REQUIRE(msv_vit_cpu_trace(t.msc.data(), isc, t.tsc.data(), t.M, t.b, t.c, t.j, cp, codes.size(), &sc, &nd, &no,
                              nd ? doms.data() : &dummy_d, no ? ops.data() : &dummy_o) == MSV_OK);
    REQUIRE(nd == doms.size() && no == ops.size());
    REQUIRE((nd == 0) == (codes.empty() || !std::isfinite(sc)));
    const uint32_t leng = t.M - 1;
    uint32_t last_i = 0;
    uint64_t at = 0;
    for (const msv_vit_domain& d : doms) {
        REQUIRE(d.ops_begin == at && d.ops_len >= 1);
        REQUIRE(last_i < d.i_from && d.i_from <= d.i_to && d.i_to <= codes.size());
        REQUIRE(1 <= d.k_from && d.k_from <= d.k_to && d.k_to <= leng);
        REQUIRE(ops[at] == 'M' && ops[at + d.ops_len - 1] == 'M');
        uint32_t i = d.i_from - 1, k = d.k_from - 1;
        for (uint64_t o = at; o < at + d.ops_len; ++o) {
            REQUIRE(ops[o] == 'M' || ops[o] == 'I' || ops[o] == 'D');
            if (ops[o] != 'D') ++i;
            if (ops[o] != 'I') ++k;
            REQUIRE(ops[o] != 'I' || k < leng);  // no I at node LENG
        }
        REQUIRE(i == d.i_to && k == d.k_to);
        last_i = d.i_to;
        at += d.ops_len;
    }
    REQUIRE(at == no);
    return nd;
}

Tables random_model(std::mt19937& rng, uint32_t leng, bool inserts) {
    Tables t;
    t.M = leng + 1;
    t.inserts = inserts;
    std::normal_distribution<float> e(0.0f, 1.5f);
    std::uniform_real_distribution<float> p(0.05f, 1.0f);
    t.msc.resize(20 * t.M);
    t.isc.resize(20 * t.M);
    t.tsc.resize(7 * t.M);
    for (auto& x : t.msc) x = e(rng);
    for (auto& x : t.isc) x = 0.5f * e(rng);
    for (uint32_t r = 0; r < 20; ++r) t.msc[r * t.M] = -std::numeric_limits<float>::infinity();
    for (auto& x : t.tsc) x = std::log(p(rng));
    t.b = std::log(2.0f / static_cast<float>(t.M * (t.M + 1)));
    t.c = t.j = std::log(0.5f);
    return t;
}

void tiny_models() {
    std::mt19937 rng(7);
    for (uint32_t leng = 1; leng <= 5; ++leng)
        for (int inserts = 0; inserts < 2; ++inserts)
            for (int trial = 0; trial < 6; ++trial) {
                Tables t = random_model(rng, leng, inserts != 0);
                if (trial == 5) t.c -= 0.75f;  // distinct exits
                for (uint32_t L = 0; L <= 5; ++L) {
                    std::vector<uint8_t> codes(L);
                    for (auto& x : codes) x = static_cast<uint8_t>(rng() % 20);
                    trace_and_check(t, codes);
                }
            }
}

void bundled_profiles(const std::string& root) {
    std::mt19937 rng(11);
    for (const char* name : {"100", "1400", "2405"}) {
        msv_hmm* hmm = nullptr;
        REQUIRE(msv_hmm_read((root + "/data/profile_HMMs/" + name + ".hmm").c_str(), &hmm) == MSV_OK);
        for (int mode = 0; mode < 2; ++mode) {
            Tables t;
            t.M = static_cast<uint32_t>(msv_hmm_model_length(hmm));
            t.inserts = mode == MSV_INSERTS_LOG_ODDS;
            t.msc.resize(20 * t.M);
            t.isc.resize(20 * t.M);
            t.tsc.resize(7 * t.M);
            REQUIRE(msv_hmm_viterbi_scores(hmm, mode, t.msc.data(), t.isc.data(), t.tsc.data(), &t.b, &t.c, &t.j) ==
                    MSV_OK);
            // a homolog: residues of the best-scoring column of a run of nodes, with a gap, between random flanks
            const float* match = msv_hmm_match_emissions(hmm);
            for (uint32_t L : {0u, 1u, 2u, 63u, 64u, 65u, 129u}) {
                std::vector<uint8_t> codes(L);
                for (auto& x : codes) x = static_cast<uint8_t>(rng() % 20);
                uint32_t k = 1 + rng() % (t.M - 1);
                for (uint32_t i = L / 4; i < L - L / 4 && k < t.M; ++i, ++k) {
                    if (i == L / 2) k += 5;  // a deletion
                    if (k >= t.M) break;
                    uint8_t best = 0;
                    for (uint8_t r = 1; r < 20; ++r)
                        if (match[k * 20 + r] > match[k * 20 + best]) best = r;
                    codes[i] = best;
                }
                const uint32_t nd = trace_and_check(t, codes);
                REQUIRE(L == 0 || nd >= 1);
            }
            // a bad residue is the score call's status, and nothing is written
            std::vector<uint8_t> bad(10, 3);
            bad[4] = 20;
            float sc = 0;
            uint32_t nd = 0;
            uint64_t no = 0;
            REQUIRE(msv_vit_cpu_trace(t.msc.data(), nullptr, t.tsc.data(), t.M, t.b, t.c, t.j, bad.data(), bad.size(), &sc,
                                      &nd, &no, nullptr, nullptr) == MSV_ERR_BAD_RESIDUE);
        }
        msv_hmm_destroy(hmm);
    }
}

void chunk_cuts() {
    std::mt19937_64 rng(13);
    for (int trial = 0; trial < 500; ++trial) {
        const uint64_t n = rng() % 40, workspace = 1 + rng() % 3000;
        std::vector<uint64_t> bytes(n), cuts(n + 1);
        uint64_t most = 0;
        for (auto& b : bytes) most = std::max(most, b = rng() % 1000);
        uint64_t chunks = 99;
        const msv_status s = msv_vit_trace_chunk_cuts(n ? bytes.data() : nullptr, n, workspace, cuts.data(), &chunks);
        if (most > workspace) {
            REQUIRE(s == MSV_ERR_OUT_OF_MEMORY);
            continue;
        }
        REQUIRE(s == MSV_OK && (chunks == 0) == (n == 0));
        REQUIRE(cuts[0] == 0 && cuts[chunks] == n);
        for (uint64_t c = 0; c < chunks; ++c) {
            REQUIRE(cuts[c] < cuts[c + 1]);
            uint64_t sum = 0;
            for (uint64_t q = cuts[c]; q < cuts[c + 1]; ++q) sum += bytes[q];
            REQUIRE(sum <= workspace);
        }
    }
    const uint64_t big[2] = {1ull << 63, 1ull << 63};
    uint64_t cuts[3], chunks = 0;
    REQUIRE(msv_vit_trace_chunk_cuts(big, 2, ~0ull, cuts, &chunks) == MSV_OK && chunks == 2);
    REQUIRE(msv_vit_trace_chunk_cuts(big, 2, (1ull << 63) - 1, cuts, &chunks) == MSV_ERR_OUT_OF_MEMORY);
}

void layout() {
    for (int i = 0; i < msv_vit_trace_plan_count(); ++i) {
        const uint32_t cap = msv_vit_trace_plan_capacity(i);
        uint32_t word, lane, shift, words, lanes;
        REQUIRE(msv_vit_trace_plan_cell(i, 1, &word, &lane, &shift, &words, &lanes) == MSV_OK);
        for (uint32_t states : {cap, cap - 1, 1u}) {
            std::vector<uint32_t> row(static_cast<size_t>(words) * lanes, 0);  // one row, every cell set once
            for (uint32_t k = 1; k <= states; ++k) {
                REQUIRE(msv_vit_trace_plan_cell(i, k, &word, &lane, &shift, nullptr, nullptr) == MSV_OK);
                REQUIRE(word < words && lane < lanes && shift <= 28);
                uint32_t& w = row[static_cast<size_t>(word) * lanes + lane];
                REQUIRE(((w >> shift) & 15u) == 0);
                w |= 15u << shift;
            }
        }
        REQUIRE(msv_vit_trace_plan_cell(i, 0, &word, &lane, &shift, &words, &lanes) == MSV_ERR_INVALID_ARGUMENT);
        REQUIRE(msv_vit_trace_plan_cell(i, cap + 1, &word, &lane, &shift, &words, &lanes) == MSV_ERR_INVALID_ARGUMENT);
        REQUIRE(msv_vit_trace_sequence_bytes(i, 400) == 400ull * (static_cast<uint64_t>(words) * lanes + 1) * 4);
    }
}

}  // namespace

int main(int argc, char** argv) {
    const std::string root = argc > 1 ? argv[1] : ".";
    tiny_models();
    bundled_profiles(root);
    chunk_cuts();
    layout();
    std::printf("sanitize_trace passed\n");
    return 0;
}
