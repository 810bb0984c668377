// sanitize_forward.cpp -- the Forward stage's host half under AddressSanitizer / UBSan (csrc/Makefile
// `asan_forward`): the float64 CPU Forward on random models and on a bundled profile, the kernel-layout odds tables
// with the D-scan constants at R = capacity, capacity - 1 and 1 real states of every variant's S, and the P-values.
// Host-only sources, its own main.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <string>
#include <vector>

#include "fwd_host.h"
#include "msv.h"

namespace {

#define REQUIRE(cond)                                                        \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                    \
        }                                                                    \
    } while (0)

struct Model {
    uint32_t M;
    std::vector<float> msc, isc, tsc;
    float b, c, j;
};

Model random_model(std::mt19937& rng, uint32_t leng) {
    Model m;
    m.M = leng + 1;
    std::normal_distribution<float> em(0.0f, 1.5f);
    std::uniform_real_distribution<float> pr(0.05f, 1.0f);
    m.msc.resize(20 * m.M);
    m.isc.resize(20 * m.M);
    m.tsc.resize(7 * m.M);
    for (float& x : m.msc) x = em(rng);
    for (float& x : m.isc) x = 0.5f * em(rng);
    for (uint32_t r = 0; r < 20; ++r) m.msc[r * m.M] = -std::numeric_limits<float>::infinity();
    for (float& x : m.tsc) x = std::log(pr(rng));
    m.b = std::log(2.0f / static_cast<float>(m.M * (m.M + 1)));
    m.c = std::log(0.5f);
    m.j = std::log(0.25f);
    return m;
}

std::vector<uint8_t> random_codes(std::mt19937& rng, size_t L) {
    std::uniform_int_distribution<int> aa(0, 19);
    std::vector<uint8_t> c(L);
    for (uint8_t& x : c) x = static_cast<uint8_t>(aa(rng));
    return c;
}

void cpu_forward(std::mt19937& rng) {
    for (uint32_t leng : {1u, 2u, 3u, 64u, 65u, 300u}) {
        const Model m = random_model(rng, leng);
        for (int ins = 0; ins < 2; ++ins)
            for (size_t L : {size_t(0), size_t(1), size_t(2), size_t(63), size_t(200)}) {
                const std::vector<uint8_t> codes = random_codes(rng, L);
                double sc = 0;
                REQUIRE(msv_fwd_cpu_score(m.msc.data(), ins ? m.isc.data() : nullptr, m.tsc.data(), m.M, m.b, m.c, m.j,
                                          codes.data(), L, &sc) == MSV_OK);
                REQUIRE(L == 0 ? std::isinf(sc) && sc < 0 : std::isfinite(sc));
            }
    }
    // a batch over host threads, a bad residue, and the float64 rescaling (more than 709 nats of odds)
    Model m = random_model(rng, 40);
    for (uint32_t k = 1; k < m.M; ++k)
        for (uint32_t r = 0; r < 20; ++r) m.msc[r * m.M + k] = 3.0f;
    std::vector<uint8_t> codes = random_codes(rng, 3000);
    std::vector<uint64_t> offsets = {0, 0, 5, 900, 3000};
    std::vector<double> out(4);
    REQUIRE(msv_fwd_cpu_score_batch(m.msc.data(), nullptr, m.tsc.data(), m.M, m.b, m.c, m.j, codes.data(),
                                    offsets.data(), 4, out.data()) == MSV_OK);
    REQUIRE(std::isinf(out[0]) && std::isfinite(out[1]) && std::isfinite(out[3]) && out[3] > 709.0);
    codes[7] = 20;
    REQUIRE(msv_fwd_cpu_score_batch(m.msc.data(), nullptr, m.tsc.data(), m.M, m.b, m.c, m.j, codes.data(),
                                    offsets.data(), 4, out.data()) == MSV_ERR_BAD_RESIDUE);
    REQUIRE(msv_fwd_cpu_score_batch(m.msc.data(), nullptr, m.tsc.data(), m.M, m.b, m.c, m.j, nullptr, offsets.data(), 0,
                                    nullptr) == MSV_OK);
}

void bundled_profile(const std::string& root, std::mt19937& rng) {
    msv_hmm* h = nullptr;
    REQUIRE(msv_hmm_read((root + "/data/profile_HMMs/100.hmm").c_str(), &h) == MSV_OK);
    const size_t M = msv_hmm_model_length(h);
    std::vector<float> msc(20 * M), isc(20 * M), tsc(7 * M);
    float b, c, j;
    REQUIRE(msv_hmm_viterbi_scores(h, MSV_INSERTS_LOG_ODDS, msc.data(), isc.data(), tsc.data(), &b, &c, &j) == MSV_OK);
    const std::vector<uint8_t> codes = random_codes(rng, 150);
    double zero = 0, odds = 0;
    REQUIRE(msv_fwd_cpu_score(msc.data(), nullptr, tsc.data(), static_cast<uint32_t>(M), b, c, j, codes.data(), 150,
                              &zero) == MSV_OK);
    REQUIRE(msv_fwd_cpu_score(msc.data(), isc.data(), tsc.data(), static_cast<uint32_t>(M), b, c, j, codes.data(), 150,
                              &odds) == MSV_OK);
    REQUIRE(std::isfinite(zero) && std::isfinite(odds));
    msv_hmm_destroy(h);
}

void table_builders(std::mt19937& rng) {
    for (int S : {2, 6, 12, 22, 38}) {
        const uint32_t capacity = 64u * static_cast<uint32_t>(S);
        for (uint32_t leng : {capacity, capacity - 1, 1u}) {
            const Model m = random_model(rng, leng);
            for (int ins = 0; ins < 2; ++ins) {
                const msv_host::FwdTables t =
                    msv_host::fwd_tables(m.msc.data(), ins ? m.isc.data() : nullptr, m.tsc.data(), m.M, S, ins != 0);
                const size_t row = static_cast<size_t>(S) * 64;
                REQUIRE(t.et.size() == 20 * row && t.tt.size() == 8 * row && t.scan.size() == 6 * 64);
                REQUIRE(t.it.size() == (ins ? 20 * row : 0));
                for (float x : t.et) REQUIRE(x >= 0.0f && std::isfinite(x));
                for (float x : t.tt) REQUIRE(x >= 0.0f && x <= 1.0f);
                for (float x : t.scan) REQUIRE(x >= 0.0f && x <= 1.0f);
                // the last real state's match odds sit where the layout says; the slot after it is padding
                const uint32_t k = leng, l = (k - 1) / S, q = (k - 1) % S;
                const size_t at = 2 * ((static_cast<size_t>(q) / 2) * 64 + l) + (q & 1);
                REQUIRE(t.et[at] == static_cast<float>(std::exp(static_cast<double>(m.msc[k]))));
                if (leng < capacity) {
                    const uint32_t k2 = leng + 1, l2 = (k2 - 1) / S, q2 = (k2 - 1) % S;
                    REQUIRE(t.et[2 * ((static_cast<size_t>(q2) / 2) * 64 + l2) + (q2 & 1)] == 0.0f);
                }
            }
            std::vector<float> dd(64 * S), prefix(64 * S), steps(6 * 64);
            REQUIRE(msv_fwd_scan_constants(m.tsc.data(), m.M, static_cast<uint32_t>(S), dd.data(), prefix.data(),
                                           steps.data()) == MSV_OK);
            REQUIRE(prefix[0] == dd[0]);
            if (leng == capacity) {
                // a closed node (tests/forward_batches.py knocked()): its d->d sits in lane 32's first slot, so that
                // lane's prefix products and every scan product over a window of lanes that holds it are exactly 0
                Model z = m;
                const uint32_t node = 32u * static_cast<uint32_t>(S);
                const float ninf = -std::numeric_limits<float>::infinity();
                for (uint32_t r = 0; r < 20; ++r) z.msc[r * z.M + node] = ninf;
                z.tsc[node * 7 + 2] = z.tsc[node * 7 + 5] = z.tsc[node * 7 + 6] = ninf;  // m->d, d->m, d->d
                REQUIRE(msv_fwd_scan_constants(z.tsc.data(), z.M, static_cast<uint32_t>(S), dd.data(), prefix.data(),
                                               steps.data()) == MSV_OK);
                for (int q = 0; q < S; ++q) REQUIRE(prefix[32 * S + q] == 0.0f);
                for (int j = 0; j < 6; ++j)
                    for (int l = 32; l < 64 && l < 32 + (1 << j); ++l) REQUIRE(steps[j * 64 + l] == 0.0f);
                for (float x : steps) REQUIRE(x >= 0.0f && x <= 1.0f);
                const std::vector<uint8_t> codes = random_codes(rng, 40);
                double sc = 0;
                REQUIRE(msv_fwd_cpu_score(z.msc.data(), nullptr, z.tsc.data(), z.M, z.b, z.c, z.j, codes.data(), 40,
                                          &sc) == MSV_OK);
                REQUIRE(std::isfinite(sc));
            }
        }
        REQUIRE(msv_fwd_scan_constants(nullptr, 2, static_cast<uint32_t>(S), nullptr, nullptr, nullptr) ==
                MSV_ERR_INVALID_ARGUMENT);
    }
}

void pvalues() {
    const std::vector<float> scores = {-std::numeric_limits<float>::infinity(), -3.5f, 40.0f,
                                       std::numeric_limits<float>::infinity()};
    const std::vector<uint64_t> offsets = {0, 0, 100, 400, 401};
    std::vector<double> p(4);
    REQUIRE(msv_fwd_pvalues(scores.data(), offsets.data(), 4, -4.0f, 0.7f, p.data()) == MSV_OK);
    REQUIRE(p[0] == 1.0 && p[1] > 0.0 && p[1] <= 1.0 && p[2] < 1e-6 && p[3] == 0.0);
    const std::vector<uint64_t> bad = {0, 5, 2};
    REQUIRE(msv_fwd_pvalues(scores.data(), bad.data(), 2, -4.0f, 0.7f, p.data()) == MSV_ERR_INVALID_ARGUMENT);
}

}  // namespace

int main(int argc, char** argv) {
    const std::string root = argc > 1 ? argv[1] : ".";
    std::mt19937 rng(12345);
    cpu_forward(rng);
    bundled_profile(root, rng);
    table_builders(rng);
    pvalues();
    std::printf("sanitize_forward passed\n");
    return 0;
}
