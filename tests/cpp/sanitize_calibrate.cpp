// sanitize_calibrate.cpp -- the calibration stage's host half under AddressSanitizer / UBSan (csrc/Makefile
// `asan_calibrate`): lambda of a bundled profile, the thresholds and the draw at its edges, the null sample by slices
// (a first above 2^32, L = 1, n = 0), the two fits with every rejection of msv.h, Newton's loop driven to its failure
// status, tau, the chunk arithmetic and the options' prefix rule, and the CPU twin of the whole stage on 100.hmm.
// Host-only sources, its own main.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <string>
#include <vector>

#include "cal_host.h"
#include "msv.h"

namespace {

#define REQUIRE(cond)                                                        \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                    \
        }                                                                    \
    } while (0)

void sample() {
    const float* bg = msv_background_frequencies();
    uint32_t T[19];
    REQUIRE(msv_cal_thresholds(bg, T) == MSV_OK);
    REQUIRE(msv_cal_thresholds(nullptr, T) == MSV_ERR_INVALID_ARGUMENT);
    for (int j = 1; j < 19; ++j) REQUIRE(T[j] > T[j - 1]);
    REQUIRE(T[18] < (1u << 24));
    // the draw at every threshold's edge
    std::vector<uint32_t> draws = {0, (1u << 24) - 1};
    for (int j = 0; j < 19; ++j) {
        draws.push_back(T[j] - 1);
        draws.push_back(T[j]);
    }
    std::vector<uint8_t> codes(draws.size());
    REQUIRE(msv_cal_codes_of_draws(bg, draws.data(), draws.size(), codes.data()) == MSV_OK);
    REQUIRE(codes[0] == 0 && codes[1] == 19);
    for (int j = 0; j < 19; ++j) REQUIRE(codes[2 + 2 * j] == j && codes[3 + 2 * j] == j + 1);
    REQUIRE(msv_cal_codes_of_draws(bg, nullptr, 0, nullptr) == MSV_OK);

    for (uint64_t L : {1ull, 15ull, 16ull, 17ull, 100ull}) {
        for (uint64_t first : {0ull, 5ull, (1ull << 32) + 77ull}) {
            const uint64_t n = 7;
            std::vector<uint8_t> whole(n * L), part(3 * L);
            std::vector<uint64_t> off(n + 1), poff(4);
            REQUIRE(msv_cal_generate(bg, 42, 2, first, n, L, whole.data(), off.data()) == MSV_OK);
            REQUIRE(msv_cal_generate(bg, 42, 2, first + 4, 3, L, part.data(), poff.data()) == MSV_OK);
            REQUIRE(std::memcmp(part.data(), whole.data() + 4 * L, 3 * L) == 0);
            for (uint64_t j = 0; j <= n; ++j) REQUIRE(off[j] == j * L);
            for (uint8_t c : whole) REQUIRE(c < 20);
        }
    }
    uint64_t one = 99;
    REQUIRE(msv_cal_generate(bg, ~0ull, 0, 0, 0, 200, nullptr, &one) == MSV_OK && one == 0);
    REQUIRE(msv_cal_generate(bg, 0, 0, 0, 1, 0xffffffffull, nullptr, &one) == MSV_ERR_INVALID_ARGUMENT);
    REQUIRE(msv_cal_generate(bg, 0, 0, 0, 1, 5, nullptr, &one) == MSV_ERR_INVALID_ARGUMENT);
}

void fits() {
    std::mt19937_64 rng(7);
    std::extreme_value_distribution<double> gumbel(-8.0, 1.0 / 0.7);
    for (uint64_t n : {2ull, 3ull, 200ull, 5000ull}) {
        std::vector<float> x(n);
        for (float& v : x) v = static_cast<float>(gumbel(rng));
        if (n == 2) x[1] = x[0] + 1.0f;
        double mu = 0, lam = 0, loc = 0;
        uint32_t it = 0;
        REQUIRE(msv_cal_fit_gumbel(x.data(), n, 0, &mu, &lam, &it) == MSV_OK);
        REQUIRE(lam > 0 && std::isfinite(mu) && it >= 1 && it <= msv_host::kCalMaxIterations);
        REQUIRE(msv_cal_fit_location(x.data(), n, 0, lam, &loc) == MSV_OK && loc == mu);
        REQUIRE(msv_cal_fit_location(x.data(), n, 200, 0.7, &loc) == MSV_OK && std::isfinite(loc));
        REQUIRE(msv_cal_fit_gumbel(x.data(), n, 100, &mu, &lam, nullptr) == MSV_OK);
        if (n == 5000) REQUIRE(std::fabs(lam / 0.69314718055994529 - 0.7) < 0.05);  // bits of nats: lambda ln 2
    }
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    double mu = 0, lam = 0;
    const std::vector<std::vector<float>> bad = {{}, {1.0f}, {2.0f, 2.0f, 2.0f}, {0.0f, 1.0f, -inf}, {0.0f, inf, 1.0f},
                                                  {nan, 0.0f, 1.0f}};
    for (const auto& x : bad) {
        REQUIRE(msv_cal_fit_gumbel(x.data(), x.size(), 0, &mu, &lam, nullptr) == MSV_ERR_INVALID_ARGUMENT);
        REQUIRE(msv_cal_fit_location(x.data(), x.size(), 50, 0.7, &mu) == MSV_ERR_INVALID_ARGUMENT);
    }
    const float ok[3] = {0.0f, 1.0f, 3.0f};
    REQUIRE(msv_cal_fit_location(ok, 3, 0, 0.0, &mu) == MSV_ERR_INVALID_ARGUMENT);
    REQUIRE(msv_cal_fit_location(ok, 3, 0, -1.0, &mu) == MSV_ERR_INVALID_ARGUMENT);
    REQUIRE(msv_cal_fit_location(nullptr, 3, 0, 0.7, &mu) == MSV_ERR_INVALID_ARGUMENT);
    REQUIRE(msv_cal_fit_gumbel(ok, 3, 0, nullptr, &lam, nullptr) == MSV_ERR_INVALID_ARGUMENT);

    // Newton's loop itself: sums that never let the step shrink run the 100 iterations and fail; a lambda that leaves
    // the positive finite numbers fails at once; sums of a one-point sample (the root is 1 / ybar) converge
    uint32_t it = 0;
    double out = -1.0;
    uint32_t calls = 0;
    REQUIRE(msv_host::cal_newton(
                1.0, 1.0,
                [&](double l, double* S) {  // f / f' = +1/4, -1/4, +1/4, ..: lambda goes 1, 0.75, 1, .. for ever
                    const double step = ++calls % 2 ? 0.25 : -0.25;
                    S[0] = 1.0;
                    S[1] = 1.0;                                        // r = ybar: f = 1 / l
                    S[2] = 1.0 - 1.0 / (l * l) - 1.0 / (l * step);     // f' = r^2 - S2 - 1 / l^2 = f / step
                },
                &out, &it) == MSV_ERR_NO_CONVERGENCE);
    REQUIRE(it == msv_host::kCalMaxIterations && calls == msv_host::kCalMaxIterations && out == -1.0);
    REQUIRE(msv_host::cal_newton(1.0, std::numeric_limits<double>::infinity(), [](double, double*) { std::abort(); },
                                 &out, &it) == MSV_ERR_NO_CONVERGENCE && it == 0);
    REQUIRE(msv_host::cal_newton(1.0, -1.0, [](double, double*) { std::abort(); }, &out, &it) ==
            MSV_ERR_NO_CONVERGENCE);
    REQUIRE(msv_host::cal_newton(
                2.0, 5.0,  // 5 > 2 / ybar: the first step would leave the positive numbers and is a halving
                [](double, double* S) {
                    S[0] = 1.0;
                    S[1] = S[2] = 0.0;
                },
                &out, &it) == MSV_OK);
    REQUIRE(std::fabs(out - 0.5) < 1e-12 && it < 20);

    double tau = 0;
    REQUIRE(msv_cal_tau(-1.75, 1.22, 0.7175, 0.04, &tau) == MSV_OK);
    REQUIRE(std::fabs(tau - (-1.75 - std::log(-std::log(0.96)) / 1.22 + std::log(0.04) / 0.7175)) < 1e-12);
    REQUIRE(msv_cal_tau(-1.75, 1.22, 0.7175, 0.0, &tau) == MSV_ERR_INVALID_ARGUMENT);
    REQUIRE(msv_cal_tau(-1.75, 1.22, 0.7175, 1.0, &tau) == MSV_ERR_INVALID_ARGUMENT);
    REQUIRE(msv_cal_tau(-1.75, 1.22, 0.7175, 0.04, nullptr) == MSV_ERR_INVALID_ARGUMENT);
}

void arithmetic() {
    REQUIRE(msv_cal_workspace_bytes(0, 200) == 8);
    REQUIRE(msv_cal_workspace_bytes(1, 1) == 16 + 16);
    REQUIRE(msv_cal_workspace_bytes(200, 200) == 40000 + 8 * 201);
    for (uint64_t L : {1ull, 17ull, 200ull, (1ull << 31) - 1}) {
        for (uint64_t budget : {0ull, 23ull, 24ull, 1000ull, 1ull << 20, 1ull << 40}) {
            const uint64_t n = msv_host::cal_chunk_sequences(budget, L);
            if (n) {
                REQUIRE(msv_cal_workspace_bytes(n, L) <= budget);
                REQUIRE(n * L < (1ull << 32) - (1ull << 20));
            } else {
                REQUIRE(msv_cal_workspace_bytes(1, L) > budget || L >= (1ull << 32) - (1ull << 20));
            }
        }
    }
    REQUIRE(msv_host::cal_chunk_sequences(1ull << 40, 0) == 0);

    msv_host::CalPlan plan;
    REQUIRE(msv_host::cal_plan(nullptr, 7, &plan));
    REQUIRE(plan.n[0] == 200 && plan.L[2] == 100 && plan.tail == 0.04 && plan.seed == 42);
    msv_cal_options o;
    std::memset(&o, 0, sizeof(o));
    o.struct_size = 4;
    REQUIRE(!msv_host::cal_plan(&o, 7, &plan));
    o.struct_size = offsetof(msv_cal_options, length);  // a caller built before `length`: only n is read
    o.n[1] = 64;
    o.length[1] = 9999;
    REQUIRE(msv_host::cal_plan(&o, 7, &plan) && plan.n[1] == 64 && plan.L[1] == 200);
    o.struct_size = sizeof(o);
    o.n[0] = 1;
    REQUIRE(!msv_host::cal_plan(&o, 1, &plan));
    REQUIRE(msv_host::cal_plan(&o, 2, &plan));  // (set 0 does not run)
    o.n[0] = 0;
    o.tail = 1.5;
    REQUIRE(!msv_host::cal_plan(&o, 7, &plan));
}

void twin(const std::string& root) {
    msv_hmm* hmm = nullptr;
    REQUIRE(msv_hmm_read((root + "/data/profile_HMMs/100.hmm").c_str(), &hmm) == MSV_OK);
    double lambda = 0;
    REQUIRE(msv_cal_lambda(msv_hmm_match_emissions(hmm), static_cast<uint32_t>(msv_hmm_model_length(hmm)),
                           msv_background_frequencies(), &lambda) == MSV_OK);
    float file[6], stats[6];
    msv_hmm_stats(hmm, file);
    REQUIRE(std::fabs(lambda - static_cast<double>(file[1])) <= 1e-5);
    REQUIRE(msv_cal_lambda(msv_hmm_match_emissions(hmm), 1, msv_background_frequencies(), &lambda) ==
            MSV_ERR_INVALID_ARGUMENT);

    std::vector<float> kept(24);
    for (int mode : {MSV_INSERTS_ZERO, MSV_INSERTS_LOG_ODDS}) {
        msv_cal_options o;
        std::memset(&o, 0, sizeof(o));
        o.struct_size = sizeof(o);
        o.n[0] = o.n[1] = o.n[2] = 24;
        o.length[0] = 60;
        o.length[1] = 33;
        o.length[2] = 17;
        o.insert_mode = mode;
        o.scores[1] = kept.data();
        msv_cal_report rep;
        std::memset(&rep, 0, sizeof(rep));
        rep.struct_size = sizeof(rep);
        std::memcpy(stats, file, sizeof(file));
        REQUIRE(msv_cal_cpu_calibrate(hmm, 7, &o, stats, &rep) == MSV_OK);
        REQUIRE(rep.ran == 7 && rep.chunks[2] == 1 && rep.n[0] == 24 && rep.length[1] == 33 && rep.seed == 42);
        for (int s = 0; s < 3; ++s) {
            REQUIRE(std::isfinite(rep.location[s]) && stats[2 * s] == static_cast<float>(rep.location[s]));
            REQUIRE(stats[2 * s + 1] == static_cast<float>(rep.lambda));
        }
        REQUIRE(rep.glam > 0 && rep.iterations >= 1);
        for (float v : kept) REQUIRE(std::isfinite(v));
        // a report of an older, shorter layout is filled up to its size only
        msv_cal_report small;
        std::memset(&small, 0x5a, sizeof(small));
        small.struct_size = offsetof(msv_cal_report, gmu);
        std::memcpy(stats, file, sizeof(file));
        REQUIRE(msv_cal_cpu_calibrate(hmm, 2, &o, stats, &small) == MSV_OK);
        REQUIRE(small.ran == 2 && small.location[1] == rep.location[1]);
        uint64_t pattern;
        std::memset(&pattern, 0x5a, sizeof(pattern));
        REQUIRE(std::memcmp(&small.gmu, &pattern, sizeof(pattern)) == 0);
        REQUIRE(stats[0] == file[0] && stats[4] == file[4] && stats[5] == file[5]);
    }
    std::memcpy(stats, file, sizeof(file));
    REQUIRE(msv_cal_cpu_calibrate(hmm, 0, nullptr, stats, nullptr) == MSV_OK);
    REQUIRE(std::memcmp(stats, file, sizeof(file)) == 0);
    REQUIRE(msv_cal_cpu_calibrate(hmm, 8, nullptr, stats, nullptr) == MSV_ERR_INVALID_ARGUMENT);
    REQUIRE(msv_cal_cpu_calibrate(nullptr, 7, nullptr, stats, nullptr) == MSV_ERR_INVALID_ARGUMENT);
    msv_hmm_destroy(hmm);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) {
        std::fprintf(stderr, "usage: %s <repository root>\n", argv[0]);
        return 2;
    }
    sample();
    fits();
    arithmetic();
    twin(argv[1]);
    std::printf("sanitize_calibrate passed\n");
    return 0;
}
