// sanitize_null2.cpp -- the bias stage's host half under AddressSanitizer / UBSan (csrc/Makefile `asan_null2`): the
// float64 null2 by expectation on random models (LENG 1 and Le 1 among others, another configured length, NULL
// outputs, the zero-score model), the definition of the correction on exactly sized buffers, the bias / bit score /
// P-value arithmetic with and without sequences, and the argument classes.  Host-only sources, its own main.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <vector>

#include "msv.h"
#include "null2_host.h"

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

Model random_model(std::mt19937& rng, uint32_t leng, bool flat) {
    Model m;
    m.M = leng + 1;
    std::normal_distribution<float> em(0.0f, 1.5f);
    std::uniform_real_distribution<float> pr(0.05f, 1.0f);
    m.msc.resize(20 * m.M);
    m.isc.resize(20 * m.M);
    m.tsc.resize(7 * m.M);
    for (float& x : m.msc) x = flat ? 0.0f : em(rng);
    for (float& x : m.isc) x = flat ? 0.0f : 0.5f * em(rng);
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

void null2_and_correction(std::mt19937& rng) {
    for (uint32_t leng : {1u, 2u, 3u, 64u, 65u, 130u})
        for (int flat = 0; flat < 2; ++flat) {
            const Model m = random_model(rng, leng, flat != 0);
            for (int pass = 0; pass < 2; ++pass) {
                const float* isc = pass ? m.isc.data() : nullptr;
                for (size_t Le : {size_t(1), size_t(2), size_t(17), size_t(90)}) {
                    const std::vector<uint8_t> codes = random_codes(rng, Le);  // exactly sized
                    for (size_t Lc : {Le, Le + 300}) {
                        std::vector<double> n2(msv_host::kNull2Residues);
                        double dc = 0;
                        REQUIRE(msv_aln_cpu_null2(m.msc.data(), isc, m.tsc.data(), m.M, m.b, m.c, m.j, codes.data(), Le,
                                                  Lc, n2.data(), &dc) == MSV_OK);
                        REQUIRE(msv_aln_cpu_null2(m.msc.data(), isc, m.tsc.data(), m.M, m.b, m.c, m.j, codes.data(), Le,
                                                  Lc, nullptr, nullptr) == MSV_OK);
                        std::vector<float> f2(n2.begin(), n2.end());
                        for (double x : n2) REQUIRE(std::isfinite(x) && x > 0.0);
                        if (flat) {
                            for (double x : n2) REQUIRE(std::fabs(x - 1.0) <= 1e-12);
                            REQUIRE(std::fabs(dc) <= 1e-12);
                        }
                        float fdc = 0;
                        REQUIRE(msv_aln_null2_correction(f2.data(), codes.data(), Le, &fdc) == MSV_OK);
                        REQUIRE(std::fabs(static_cast<double>(fdc) - dc) <= 1e-5 * (1.0 + std::fabs(dc)));
                    }
                }
            }
        }
    const Model m = random_model(rng, 5, false);
    const std::vector<uint8_t> bad = {1, 2, 20};
    double dc = 0;
    float fdc = 0;
    const std::vector<float> ones(msv_host::kNull2Residues, 1.0f);
    REQUIRE(msv_aln_cpu_null2(m.msc.data(), nullptr, m.tsc.data(), m.M, m.b, m.c, m.j, bad.data(), 3, 3, nullptr, &dc) ==
            MSV_ERR_BAD_RESIDUE);
    REQUIRE(msv_aln_cpu_null2(m.msc.data(), nullptr, m.tsc.data(), m.M, m.b, m.c, m.j, bad.data(), 2, 1, nullptr, &dc) ==
            MSV_ERR_INVALID_ARGUMENT);
    REQUIRE(msv_aln_cpu_null2(m.msc.data(), nullptr, m.tsc.data(), m.M, m.b, m.c, m.j, bad.data(), 0, 0, nullptr, &dc) ==
            MSV_ERR_INVALID_ARGUMENT);
    REQUIRE(msv_aln_null2_correction(ones.data(), bad.data(), 3, &fdc) == MSV_ERR_BAD_RESIDUE);
    REQUIRE(msv_aln_null2_correction(ones.data(), nullptr, 0, &fdc) == MSV_OK && fdc == 0.0f);
    REQUIRE(msv_aln_null2_correction(nullptr, bad.data(), 2, &fdc) == MSV_ERR_INVALID_ARGUMENT);
}

void bias_arithmetic(std::mt19937& rng) {
    std::normal_distribution<float> sc(20.0f, 30.0f), corr(0.0f, 6.0f);
    for (uint64_t m : {uint64_t(0), uint64_t(1), uint64_t(33)})
        for (uint64_t n_seq : {uint64_t(0), uint64_t(1), uint64_t(7)}) {
            std::vector<uint64_t> lens(n_seq), Le(m), Lc(m);
            std::vector<uint32_t> parent(m);
            std::vector<float> env(m), dc(m), fwd(n_seq);
            for (uint64_t s = 0; s < n_seq; ++s) {
                lens[s] = s == 0 && n_seq > 1 ? 0 : 1 + rng() % 2000;
                fwd[s] = sc(rng);
            }
            for (uint64_t q = 0; q < m; ++q) {
                parent[q] = n_seq > 1 ? 1 + static_cast<uint32_t>(rng() % (n_seq - 1)) : 0;
                Lc[q] = n_seq ? lens[parent[q]] : 1 + rng() % 2000;
                Le[q] = 1 + rng() % Lc[q];
                env[q] = sc(rng);
                dc[q] = corr(rng);
            }
            // exactly sized outputs
            std::vector<float> bias(m), bits(m), sbias(n_seq), sbits(n_seq);
            std::vector<double> pv(m), spv(n_seq);
            REQUIRE(msv_aln_bias_scores(env.data(), Le.data(), Lc.data(), dc.data(), m, parent.data(), fwd.data(),
                                        lens.data(), n_seq, -4.0f, 0.7f, bias.data(), bits.data(), pv.data(),
                                        sbias.data(), sbits.data(), spv.data()) == MSV_OK);
            REQUIRE(msv_aln_bias_scores(env.data(), Le.data(), Lc.data(), dc.data(), m, parent.data(), fwd.data(),
                                        lens.data(), n_seq, -4.0f, 0.7f, nullptr, nullptr, nullptr, nullptr, nullptr,
                                        nullptr) == MSV_OK);
            for (uint64_t q = 0; q < m; ++q) REQUIRE(bias[q] >= 0.0f && pv[q] >= 0.0 && pv[q] <= 1.0);
            for (uint64_t s = 0; s < n_seq; ++s) REQUIRE(sbias[s] >= 0.0f && spv[s] >= 0.0 && spv[s] <= 1.0);
            if (m && n_seq) {
                parent[0] = static_cast<uint32_t>(n_seq);
                REQUIRE(msv_aln_bias_scores(env.data(), Le.data(), Lc.data(), dc.data(), m, parent.data(), fwd.data(),
                                            lens.data(), n_seq, -4.0f, 0.7f, bias.data(), bits.data(), pv.data(),
                                            sbias.data(), sbits.data(), spv.data()) == MSV_ERR_INVALID_ARGUMENT);
            }
        }
}

}  // namespace

int main() {
    std::mt19937 rng(20250712);
    null2_and_correction(rng);
    bias_arithmetic(rng);
    std::printf("sanitize_null2 passed\n");
    return 0;
}
