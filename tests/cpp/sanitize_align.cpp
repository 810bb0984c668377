// sanitize_align.cpp -- the alignment stage's host half under AddressSanitizer / UBSan (csrc/Makefile `asan_align`):
// the float64 envelope decode on random models (LENG 1, Le 0 and Le 1 among others, another configured length, NULL
// outputs), the definition of the optimal-accuracy alignment by its two-call protocol (with closed transitions and
// with counts that are too small), the twin, the gate bytes of every variant's S and the workspace arithmetic with
// the chunk cuts.  Host-only sources, its own main.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <vector>

#include "aln_host.h"
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

void decode_and_definition(std::mt19937& rng) {
    const float ninf = -std::numeric_limits<float>::infinity();
    for (uint32_t leng : {1u, 2u, 3u, 64u, 65u, 130u}) {
        Model m = random_model(rng, leng);
        for (int pass = 0; pass < 3; ++pass) {
            const float* isc = pass ? m.isc.data() : nullptr;
            if (pass == 2) {  // a closed node, and no way from E to J
                if (leng >= 3)
                    for (int t = 0; t < 7; ++t) m.tsc[2 * 7 + t] = ninf;
                m.j = ninf;
            }
            for (size_t Le : {size_t(0), size_t(1), size_t(2), size_t(63), size_t(90)}) {
                const std::vector<uint8_t> codes = random_codes(rng, Le);
                for (size_t Lc : {Le, Le + 300}) {
                    const size_t M = m.M;
                    std::vector<double> pm(Le * M), pi(Le * M), pn(Le), pj(Le), pc(Le);
                    double score = 0;
                    REQUIRE(msv_aln_cpu_decode(m.msc.data(), isc, m.tsc.data(), m.M, m.b, m.c, m.j, codes.data(), Le, Lc,
                                               &score, pm.data(), pi.data(), pn.data(), pj.data(), pc.data()) == MSV_OK);
                    REQUIRE(msv_aln_cpu_decode(m.msc.data(), isc, m.tsc.data(), m.M, m.b, m.c, m.j, codes.data(), Le, Lc,
                                               nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == MSV_OK);
                    if (Le == 0) {
                        REQUIRE(std::isinf(score) && score < 0);
                    } else {
                        REQUIRE(std::isfinite(score));
                        for (size_t i = 0; i < Le; ++i) {
                            double row = pn[i] + pj[i] + pc[i];
                            for (size_t k = 0; k < M; ++k) row += pm[i * M + k] + pi[i * M + k];
                            REQUIRE(std::fabs(row - 1.0) <= 1e-9);
                        }
                    }
                    std::vector<float> fm(pm.begin(), pm.end()), fi(pi.begin(), pi.end()), fn(pn.begin(), pn.end()),
                        fj(pj.begin(), pj.end()), fc(pc.begin(), pc.end());
                    float oa = 0;
                    uint32_t nd = 0;
                    uint64_t no = 0;
                    REQUIRE(msv_aln_oa(fm.data(), fi.data(), fn.data(), fj.data(), fc.data(), m.tsc.data(), m.M, m.b,
                                       m.c, m.j, Le, Lc, &oa, &nd, &no, nullptr, nullptr, nullptr) == MSV_OK);
                    REQUIRE((Le == 0) == (nd == 0));
                    // exactly sized buffers: a write past either end is the sanitizer's to find
                    std::vector<msv_vit_domain> doms(nd);
                    std::vector<uint8_t> ops(no);
                    std::vector<float> opp(no);
                    if (nd) {
                        REQUIRE(msv_aln_oa(fm.data(), fi.data(), fn.data(), fj.data(), fc.data(), m.tsc.data(), m.M, m.b,
                                           m.c, m.j, Le, Lc, &oa, &nd, &no, doms.data(), ops.data(), opp.data()) ==
                                MSV_OK);
                        REQUIRE(nd == doms.size() && no == ops.size());
                        uint64_t at = 0;
                        for (const msv_vit_domain& d : doms) {
                            REQUIRE(d.ops_begin == at && d.ops_len >= 1 && ops[at] == 'M' && ops[at + d.ops_len - 1] == 'M');
                            REQUIRE(d.i_from >= 1 && d.i_to <= Le && d.k_from >= 1 && d.k_to <= leng);
                            at += d.ops_len;
                        }
                        REQUIRE(at == no);
                        uint32_t small = nd - 1;
                        uint64_t few = no;
                        REQUIRE(msv_aln_oa(fm.data(), fi.data(), fn.data(), fj.data(), fc.data(), m.tsc.data(), m.M, m.b,
                                           m.c, m.j, Le, Lc, &oa, &small, &few, doms.data(), ops.data(), opp.data()) ==
                                MSV_ERR_INVALID_ARGUMENT);
                    }
                    // the twin: the same bits
                    double s2 = 0;
                    float oa2 = 0;
                    uint32_t nd2 = 0;
                    uint64_t no2 = 0;
                    REQUIRE(msv_aln_cpu_align(m.msc.data(), isc, m.tsc.data(), m.M, m.b, m.c, m.j, codes.data(), Le, Lc, &s2,
                                              &oa2, &nd2, &no2, nullptr, nullptr, nullptr) == MSV_OK);
                    REQUIRE(nd2 == nd && no2 == no && (Le == 0 || (s2 == score && oa2 == oa)));
                    std::vector<msv_vit_domain> d2(nd2);
                    std::vector<uint8_t> o2(no2);
                    std::vector<float> p2(no2);
                    if (nd2) {
                        REQUIRE(msv_aln_cpu_align(m.msc.data(), isc, m.tsc.data(), m.M, m.b, m.c, m.j, codes.data(), Le, Lc,
                                                  &s2, &oa2, &nd2, &no2, d2.data(), o2.data(), p2.data()) == MSV_OK);
                        REQUIRE(o2 == ops && p2 == opp);
                    }
                }
            }
        }
    }
    const Model m = random_model(rng, 5);
    const std::vector<uint8_t> bad = {1, 2, 20};
    double s = 0;
    REQUIRE(msv_aln_cpu_decode(m.msc.data(), nullptr, m.tsc.data(), m.M, m.b, m.c, m.j, bad.data(), 3, 3, &s, nullptr,
                               nullptr, nullptr, nullptr, nullptr) == MSV_ERR_BAD_RESIDUE);
    REQUIRE(msv_aln_cpu_decode(m.msc.data(), nullptr, m.tsc.data(), m.M, m.b, m.c, m.j, bad.data(), 2, 1, &s, nullptr,
                               nullptr, nullptr, nullptr, nullptr) == MSV_ERR_INVALID_ARGUMENT);
}

void gates_and_workspace(std::mt19937& rng) {
    for (int S : {2, 6, 12, 22, 38})
        for (uint32_t leng : {static_cast<uint32_t>(64 * S), static_cast<uint32_t>(64 * S - 1), 1u}) {
            const Model m = random_model(rng, leng);
            const std::vector<uint32_t> g = msv_host::aln_gates(m.tsc.data(), m.M, m.b, S);
            REQUIRE(g.size() == static_cast<size_t>((S + 3) / 4) * 64);
            for (uint32_t k = 1; k <= 64u * static_cast<uint32_t>(S); ++k) {
                const uint32_t l = (k - 1) / static_cast<uint32_t>(S), q = (k - 1) % static_cast<uint32_t>(S);
                const uint32_t b = (g[(q / 4) * 64 + l] >> ((q % 4) * 8)) & 255u;
                if (k > leng) REQUIRE(b == 0);
                else REQUIRE((b & msv_host::kGateBM) && ((b & msv_host::kGateMM) != 0) == (k > 1) &&
                             ((b & msv_host::kGateMI) != 0) == (k < leng));
            }
        }
    for (uint32_t S : {2u, 6u, 12u, 22u, 38u})
        for (uint64_t Le : {0ull, 1ull, 129ull})
            REQUIRE(msv_aln_item_bytes(S, Le) ==
                    4 * ((Le + 1) * 6 + Le * 2 * S * 64 + Le * (((S + 7) / 8) * 64 + 1)));
    const std::vector<uint64_t> bytes = {msv_aln_item_bytes(6, 10), msv_aln_item_bytes(6, 20), msv_aln_item_bytes(6, 5)};
    std::vector<uint64_t> cuts(bytes.size() + 1);
    uint64_t n = 0;
    REQUIRE(msv_vit_trace_chunk_cuts(bytes.data(), bytes.size(), bytes[1], cuts.data(), &n) == MSV_OK && n == 3);
    REQUIRE(msv_vit_trace_chunk_cuts(bytes.data(), bytes.size(), bytes[1] - 1, cuts.data(), &n) == MSV_ERR_OUT_OF_MEMORY);
    REQUIRE(msv_vit_trace_chunk_cuts(bytes.data(), 0, 1, cuts.data(), &n) == MSV_OK && n == 0);
}

}  // namespace

int main() {
    std::mt19937 rng(20250611);
    decode_and_definition(rng);
    gates_and_workspace(rng);
    std::printf("sanitize_align passed\n");
    return 0;
}
