// sanitize_bias.cpp -- the bias filter's host half under AddressSanitizer / UBSan (csrc/Makefile `asan_bias`): the
// float64 definition on exactly sized buffers (L = 0, 1, long, homopolymers, an extreme composition, LENG 1), the
// batch form over CSR offsets with empty sequences, the filtered P-values of both tails with edge scores, the device
// table and its range refusal, and the argument classes.  Host-only sources, its own main.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "bias_filter_host.h"
#include "msv.h"

namespace {

#define REQUIRE(cond)                                                              \
    do {                                                                           \
        if (!(cond)) {                                                             \
            std::fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                          \
        }                                                                          \
    } while (0)

std::vector<float> random_compo(std::mt19937& rng, float lo, float hi, const float* f) {
    std::uniform_real_distribution<float> u(std::log(lo), std::log(hi));
    std::vector<float> c(20);
    double total = 0;
    for (int x = 0; x < 20; ++x) total += c[x] = f[x] * std::exp(u(rng));
    for (float& v : c) v = static_cast<float>(v / total);
    return c;
}

}  // namespace

int main() {
    std::mt19937 rng(20261020);
    const float* f = msv_background_frequencies();
    const float inf = std::numeric_limits<float>::infinity();
    for (uint32_t leng : {1u, 7u, 8u, 100u, 2405u, 1u << 20}) {
        const std::vector<float> compo = random_compo(rng, 0.05f, 20.0f, f);
        for (size_t L : {size_t(0), size_t(1), size_t(2), size_t(17), size_t(1025), size_t(50000)}) {
            std::vector<uint8_t> codes(L);  // exactly sized: a read past the end is an ASan report
            for (auto& c : codes) c = static_cast<uint8_t>(rng() % 20);
            double bias = -1;
            REQUIRE(msv_bf_cpu_score(compo.data(), f, leng + 1, L ? codes.data() : nullptr, L, &bias) == MSV_OK);
            REQUIRE(std::isfinite(bias));
            if (L == 0) REQUIRE(bias == 0.0);
            if (L) {
                std::fill(codes.begin(), codes.end(), uint8_t(3));  // a homopolymer
                REQUIRE(msv_bf_cpu_score(compo.data(), f, leng + 1, codes.data(), L, &bias) == MSV_OK);
                REQUIRE(std::isfinite(bias));
                codes[L - 1] = 20;
                REQUIRE(msv_bf_cpu_score(compo.data(), f, leng + 1, codes.data(), L, &bias) == MSV_ERR_BAD_RESIDUE);
            }
        }
        // compo = background: every path has the odds of its transitions, which sum to 1
        double bias = -1;
        std::vector<uint8_t> codes(500, 7);
        REQUIRE(msv_bf_cpu_score(f, f, leng + 1, codes.data(), codes.size(), &bias) == MSV_OK);
        REQUIRE(std::fabs(bias) <= 1e-12);
        float table[26];
        REQUIRE(msv_bf_device_table(compo.data(), f, leng + 1, table) == MSV_OK);
        REQUIRE(std::fabs(table[0] + table[1] - 1.0f) < 1e-6f && std::fabs(table[2] + table[3] - 1.0f) < 1e-6f);
    }
    // the batch form: empty sequences among others, and offsets that do not start at 0
    {
        const std::vector<float> compo = random_compo(rng, 0.3f, 3.0f, f);
        std::vector<uint64_t> off = {5, 5, 9, 9, 30, 30};
        std::vector<uint8_t> codes(30);
        for (auto& c : codes) c = static_cast<uint8_t>(rng() % 20);
        std::vector<double> bias(5, -1);
        REQUIRE(msv_bf_cpu_score_batch(compo.data(), f, 101, codes.data(), off.data(), 5, bias.data()) == MSV_OK);
        REQUIRE(bias[0] == 0.0 && bias[2] == 0.0 && bias[4] == 0.0);
        double one = 0;
        REQUIRE(msv_bf_cpu_score(compo.data(), f, 101, codes.data() + 9, 21, &one) == MSV_OK);
        REQUIRE(one == bias[3]);
        REQUIRE(msv_bf_cpu_score_batch(compo.data(), f, 101, nullptr, nullptr, 0, nullptr) == MSV_OK);
        off[2] = 3;  // decreasing
        REQUIRE(msv_bf_cpu_score_batch(compo.data(), f, 101, codes.data(), off.data(), 5, bias.data()) ==
                MSV_ERR_INVALID_ARGUMENT);
    }
    // the filtered P-values: zero bias is msv_pvalue_of / fwd_pvalue_of; edge scores; monotone in the bias
    {
        const std::vector<uint64_t> off = {0, 0, 1, 400, 401, 100000, 100000};
        const std::vector<float> sc = {-inf, 3.5f, -inf, -700.0f, 250.0f, 1.0f};
        const std::vector<float> zero(6, 0.0f);
        std::vector<float> b = {0.0f, 2.0f, inf, -1.0f, 100.0f, 0.5f};
        std::vector<double> p(6), q(6);
        for (int kind : {MSV_BF_GUMBEL, MSV_BF_EXPONENTIAL}) {
            REQUIRE(msv_bf_pvalues(sc.data(), zero.data(), off.data(), 6, -8.5f, 0.7f, kind, p.data()) == MSV_OK);
            REQUIRE(msv_bf_pvalues(sc.data(), b.data(), off.data(), 6, -8.5f, 0.7f, kind, q.data()) == MSV_OK);
            for (int i = 0; i < 6; ++i) {
                REQUIRE(p[i] >= 0.0 && p[i] <= 1.0 && q[i] >= 0.0 && q[i] <= 1.0);
                const double want = kind == MSV_BF_GUMBEL
                                        ? (off[i + 1] == off[i] ? 1.0 : -1.0)
                                        : msv_host::fwd_pvalue_of(sc[i], off[i + 1] - off[i], -8.5f, 0.7f);
                if (want >= 0.0) REQUIRE(std::memcmp(&want, &p[i], sizeof(double)) == 0);
                if (b[i] >= 0.0f) REQUIRE(q[i] >= p[i]);
            }
            REQUIRE(p[0] == 1.0 && q[2] == 1.0);  // empty; -inf with a +inf bias
        }
        REQUIRE(msv_bf_pvalues(sc.data(), b.data(), off.data(), 6, -8.5f, 0.7f, 2, q.data()) == MSV_ERR_INVALID_ARGUMENT);
        REQUIRE(msv_bf_pvalues(nullptr, nullptr, nullptr, 0, 0.0f, 1.0f, MSV_BF_GUMBEL, nullptr) == MSV_OK);
    }
    // the argument classes
    {
        std::vector<float> compo(f, f + 20);
        double bias = 0;
        float table[26];
        const uint8_t code = 0;
        REQUIRE(msv_bf_cpu_score(nullptr, f, 101, &code, 1, &bias) == MSV_ERR_INVALID_ARGUMENT);
        REQUIRE(msv_bf_cpu_score(compo.data(), f, 1, &code, 1, &bias) == MSV_ERR_INVALID_ARGUMENT);
        REQUIRE(msv_bf_cpu_score(compo.data(), f, 101, nullptr, 1, &bias) == MSV_ERR_INVALID_ARGUMENT);
        REQUIRE(msv_bf_cpu_score(compo.data(), f, 101, &code, 1, nullptr) == MSV_ERR_INVALID_ARGUMENT);
        compo[4] = std::numeric_limits<float>::quiet_NaN();
        REQUIRE(msv_bf_cpu_score(compo.data(), f, 101, &code, 1, &bias) == MSV_ERR_INVALID_ARGUMENT);
        compo[4] = 0.0f;  // the definition takes a zero, the float32 kernel's table does not
        REQUIRE(msv_bf_cpu_score(compo.data(), f, 101, &code, 1, &bias) == MSV_OK);
        REQUIRE(msv_bf_device_table(compo.data(), f, 101, table) == MSV_ERR_UNSUPPORTED_MODEL);
        compo[4] = 100.0f;
        REQUIRE(msv_bf_device_table(compo.data(), f, 101, table) == MSV_ERR_UNSUPPORTED_MODEL);
        compo[4] = f[4];
        REQUIRE(msv_bf_device_table(compo.data(), f, 101, nullptr) == MSV_ERR_INVALID_ARGUMENT);
        std::vector<float> bg(f, f + 20);
        bg[0] = 0.0f;
        REQUIRE(msv_bf_cpu_score(compo.data(), bg.data(), 101, &code, 1, &bias) == MSV_ERR_INVALID_ARGUMENT);
    }
    std::printf("sanitize_bias passed\n");
    return 0;
}
