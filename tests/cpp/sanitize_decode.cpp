// sanitize_decode.cpp -- the domain stage's host half under AddressSanitizer / UBSan (csrc/Makefile `asan_decode`):
// the float64 Forward / Backward decode on random models (edge lengths, a batch over host threads, the rescaling),
// the envelope rule by its two-call protocol, the Backward tables with the mirrored D-scan constants at
// R = capacity, capacity - 1 and 1 real states of every variant's S, and the workspace arithmetic with the chunk
// cuts.  Host-only sources, its own main.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <string>
#include <vector>

#include "dom_host.h"
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

void cpu_decode(std::mt19937& rng) {
    for (uint32_t leng : {1u, 2u, 3u, 64u, 65u, 300u}) {
        const Model m = random_model(rng, leng);
        for (int ins = 0; ins < 2; ++ins)
            for (size_t L : {size_t(0), size_t(1), size_t(2), size_t(63), size_t(200)}) {
                const std::vector<uint8_t> codes = random_codes(rng, L);
                std::vector<double> begin(L), end(L), occ(L);
                double f = 0, b = 0;
                REQUIRE(msv_dom_cpu_decode(m.msc.data(), ins ? m.isc.data() : nullptr, m.tsc.data(), m.M, m.b, m.c, m.j,
                                           codes.data(), L, &f, &b, begin.data(), end.data(), occ.data()) == MSV_OK);
                if (L == 0) {
                    REQUIRE(std::isinf(f) && f < 0 && std::isinf(b) && b < 0);
                    continue;
                }
                REQUIRE(std::isfinite(f) && std::fabs(f - b) <= 1e-9 * std::fmax(1.0, std::fabs(f)));
                double sb = 0, se = 0;
                for (size_t i = 0; i < L; ++i) {
                    REQUIRE(begin[i] >= 0 && end[i] >= 0 && occ[i] >= -1e-12 && occ[i] <= 1.0 + 1e-12);
                    sb += begin[i];
                    se += end[i];
                }
                REQUIRE(std::fabs(sb - se) <= 1e-9 * std::fmax(1.0, sb));
                // scores alone (every per-residue output NULL)
                double f2 = 0;
                REQUIRE(msv_dom_cpu_decode(m.msc.data(), ins ? m.isc.data() : nullptr, m.tsc.data(), m.M, m.b, m.c, m.j,
                                           codes.data(), L, &f2, nullptr, nullptr, nullptr, nullptr) == MSV_OK);
                REQUIRE(f2 == f);
            }
    }
    // a batch over host threads from a CSR that does not start at 0, a bad residue, and the rescaling of both passes
    Model m = random_model(rng, 40);
    for (uint32_t k = 1; k < m.M; ++k)
        for (uint32_t r = 0; r < 20; ++r) m.msc[r * m.M + k] = 3.0f;
    std::vector<uint8_t> codes = random_codes(rng, 3000);
    std::vector<uint64_t> offsets = {10, 10, 15, 900, 3000};
    std::vector<double> f(4), b(4), begin(2990), end(2990), occ(2990);
    REQUIRE(msv_dom_cpu_decode_batch(m.msc.data(), nullptr, m.tsc.data(), m.M, m.b, m.c, m.j, codes.data(),
                                     offsets.data(), 4, f.data(), b.data(), begin.data(), end.data(),
                                     occ.data()) == MSV_OK);
    REQUIRE(std::isinf(f[0]) && std::isfinite(f[1]) && f[3] > 709.0 && std::fabs(f[3] - b[3]) <= 1e-9 * f[3]);
    codes[17] = 20;
    REQUIRE(msv_dom_cpu_decode_batch(m.msc.data(), nullptr, m.tsc.data(), m.M, m.b, m.c, m.j, codes.data(),
                                     offsets.data(), 4, f.data(), b.data(), nullptr, nullptr,
                                     nullptr) == MSV_ERR_BAD_RESIDUE);
    REQUIRE(msv_dom_cpu_decode_batch(m.msc.data(), nullptr, m.tsc.data(), m.M, m.b, m.c, m.j, nullptr, offsets.data(),
                                     0, nullptr, nullptr, nullptr, nullptr, nullptr) == MSV_OK);
}

void regions() {
    // two regions back to back and one left open at L
    const std::vector<float> occ = {0.0f, 0.3f, 0.9f, 0.9f, 0.2f, 0.9f, 0.9f, 0.05f, 0.9f, 0.9f};
    const std::vector<float> begin = {0.0f, 0.3f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.8f, 0.0f};
    const std::vector<float> end = {0.0f, 0.0f, 0.0f, 0.85f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    uint32_t n = 0;
    REQUIRE(msv_dom_regions(begin.data(), end.data(), occ.data(), occ.size(), 0.25f, 0.10f, &n, nullptr) == MSV_OK);
    REQUIRE(n == 2);
    std::vector<msv_dom_region> r(n);
    REQUIRE(msv_dom_regions(begin.data(), end.data(), occ.data(), occ.size(), 0.25f, 0.10f, &n, r.data()) == MSV_OK);
    REQUIRE(r[0].i_from == 2 && r[0].i_to == 4 && r[1].i_from == 5 && r[1].i_to == 8);
    REQUIRE(msv_dom_regions(nullptr, nullptr, nullptr, 0, 0.25f, 0.10f, &n, nullptr) == MSV_OK && n == 0);
    REQUIRE(msv_dom_regions(nullptr, end.data(), occ.data(), 3, 0.25f, 0.10f, &n, nullptr) == MSV_ERR_INVALID_ARGUMENT);
}

void table_builders(std::mt19937& rng) {
    for (int S : {2, 6, 12, 22, 38}) {
        const uint32_t capacity = 64u * static_cast<uint32_t>(S);
        for (uint32_t leng : {capacity, capacity - 1, 1u}) {
            const Model m = random_model(rng, leng);
            for (int ins = 0; ins < 2; ++ins) {
                const msv_host::DomTables t =
                    msv_host::dom_tables(m.msc.data(), ins ? m.isc.data() : nullptr, m.tsc.data(), m.M, S, ins != 0);
                const size_t row = static_cast<size_t>(S) * 64;
                REQUIRE(t.fwd.et.size() == 20 * row && t.bt.size() == 8 * row && t.bscan.size() == 6 * 64);
                for (float x : t.bt) REQUIRE(x >= 0.0f && x <= 1.0f);
                for (float x : t.bscan) REQUIRE(x >= 0.0f && x <= 1.0f);
            }
            std::vector<float> dd(64 * S), suffix(64 * S), steps(6 * 64);
            REQUIRE(msv_dom_scan_constants(m.tsc.data(), m.M, static_cast<uint32_t>(S), dd.data(), suffix.data(),
                                           steps.data()) == MSV_OK);
            REQUIRE(suffix[S - 1] == dd[S - 1]);
            // node LENG and the padding have no transitions: the last real state's slot and all behind it hold 0
            for (uint32_t k = leng; k <= capacity; ++k) REQUIRE(dd[k - 1] == 0.0f);
            if (leng >= 3) REQUIRE(dd[leng - 2] == static_cast<float>(std::exp(static_cast<double>(m.tsc[(leng - 1) * 7 + 6]))));
        }
        REQUIRE(msv_dom_scan_constants(nullptr, 2, static_cast<uint32_t>(S), nullptr, nullptr, nullptr) ==
                MSV_ERR_INVALID_ARGUMENT);
    }
}

void workspace() {
    REQUIRE(msv_dom_sequence_bytes(0) == 24 && msv_dom_sequence_bytes(100) == 24 * 101);
    const std::vector<uint64_t> bytes = {msv_dom_sequence_bytes(10), msv_dom_sequence_bytes(20),
                                         msv_dom_sequence_bytes(5), msv_dom_sequence_bytes(40)};
    std::vector<uint64_t> cuts(bytes.size() + 1);
    uint64_t chunks = 0;
    REQUIRE(msv_vit_trace_chunk_cuts(bytes.data(), bytes.size(), 24 * 41, cuts.data(), &chunks) == MSV_OK);
    REQUIRE(chunks == 2 && cuts[0] == 0 && cuts[1] == 3 && cuts[2] == 4);  // 11 + 21 + 6 rows fit, 41 fill a chunk
    REQUIRE(msv_vit_trace_chunk_cuts(bytes.data(), bytes.size(), 24 * 40, cuts.data(), &chunks) ==
            MSV_ERR_OUT_OF_MEMORY);
}

}  // namespace

int main(int, char**) {
    std::mt19937 rng(54321);
    cpu_decode(rng);
    regions();
    table_builders(rng);
    workspace();
    std::printf("sanitize_decode passed\n");
    return 0;
}
