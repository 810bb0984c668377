// sanitize_split.cpp -- the split stage's host half under AddressSanitizer / UBSan (csrc/Makefile `asan_split`): the
// float64 Forward twin with D on random models (LENG 1, Le 0 and Le 1 among others, another configured length, NULL
// outputs), the definition of a sample by its two-call protocol on the twin's matrix rounded to float32 (with closed
// transitions, with a matrix of zeros that truncates every sample, with counts that are too small), the random
// numbers' key, the clustering with its options and thresholds, the region test and the workspace arithmetic with the
// chunk cuts.  Host-only sources, its own main.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "msv.h"
#include "spl_host.h"

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

void forward_and_samples(std::mt19937& rng) {
    const float ninf = -std::numeric_limits<float>::infinity();
    for (uint32_t leng : {1u, 2u, 3u, 64u, 65u, 130u}) {
        Model m = random_model(rng, leng);
        const size_t M = m.M;
        for (int pass = 0; pass < 3; ++pass) {
            const float* isc = pass ? m.isc.data() : nullptr;
            if (pass == 2) {  // a closed node, and no way from E to J
                if (leng >= 3)
                    for (int t = 0; t < 7; ++t) m.tsc[2 * 7 + t] = ninf;
                m.j = ninf;
            }
            for (size_t Le : {size_t(0), size_t(1), size_t(2), size_t(63), size_t(90)}) {
                const std::vector<uint8_t> codes = random_codes(rng, Le);
                const uint64_t Lc = Le + (pass == 1 ? 17 : 0);
                double score = 0;
                std::vector<double> fM(Le * M), fI(Le * M), fD(Le * M), sp((Le + 1) * 5);
                std::vector<int32_t> ex(Le + 1);
                REQUIRE(msv_spl_cpu_forward(m.msc.data(), isc, m.tsc.data(), m.M, m.b, m.c, m.j, codes.data(), Le, Lc,
                                            &score, fM.data(), fI.data(), fD.data(), sp.data(), ex.data()) == MSV_OK);
                REQUIRE(msv_spl_cpu_forward(m.msc.data(), isc, m.tsc.data(), m.M, m.b, m.c, m.j, codes.data(), Le, Lc,
                                            &score, nullptr, nullptr, nullptr, nullptr, nullptr) == MSV_OK);
                if (Le == 0) {
                    REQUIRE(std::isinf(score) && score < 0);
                    continue;
                }
                // the score agrees with the alignment-free Forward of the same envelope when Lc = Le
                if (Lc == Le) {
                    double f = 0;
                    REQUIRE(msv_fwd_cpu_score(m.msc.data(), isc, m.tsc.data(), m.M, m.b, m.c, m.j, codes.data(), Le,
                                              &f) == MSV_OK);
                    REQUIRE(std::fabs(f - score) <= 1e-9 * std::fmax(1.0, std::fabs(f)));
                }
                // rounded to float32 once (these rows stay far below 2^127: exponent as the twin's)
                std::vector<float> gM(fM.begin(), fM.end()), gI(fI.begin(), fI.end()), gD(fD.begin(), fD.end());
                std::vector<uint32_t> rec((Le + 1) * 6);
                for (size_t i = 0; i <= Le; ++i) {
                    for (int w = 0; w < 5; ++w) {
                        const float x = static_cast<float>(sp[i * 5 + static_cast<size_t>(w)]);
                        std::memcpy(&rec[i * 6 + static_cast<size_t>(w)], &x, 4);
                    }
                    rec[i * 6 + 5] = static_cast<uint32_t>(ex[i]);
                }
                const uint32_t i_from = 5, i_to = static_cast<uint32_t>(i_from + Le - 1);
                const uint64_t Lp = Lc + i_from - 1;
                for (uint32_t sample = 0; sample < 40; ++sample) {
                    uint32_t ns = 0;
                    uint64_t no = 0;
                    int trunc = -1;
                    REQUIRE(msv_spl_sample(gM.data(), gI.data(), gD.data(), rec.data(), m.tsc.data(), m.M, m.b, m.c,
                                           m.j, Lp, 42, 3, i_from, i_to, sample, &ns, &no, &trunc, nullptr, nullptr,
                                           nullptr) == MSV_OK);
                    REQUIRE(trunc == 0 || trunc == 1);
                    std::vector<msv_spl_segment> seg(ns);
                    std::vector<msv_vit_domain> dom(ns);
                    std::vector<uint8_t> ops(no);
                    uint32_t ns2 = ns;
                    uint64_t no2 = no;
                    REQUIRE(msv_spl_sample(gM.data(), gI.data(), gD.data(), rec.data(), m.tsc.data(), m.M, m.b, m.c,
                                           m.j, Lp, 42, 3, i_from, i_to, sample, &ns2, &no2, &trunc, seg.data(),
                                           dom.data(), ops.data()) == MSV_OK);
                    REQUIRE(ns2 == ns && no2 == no);
                    if (pass == 2) REQUIRE(ns <= 1);  // no J: one domain at the most
                    uint64_t at = 0;
                    uint32_t prev = i_from - 1;
                    for (uint32_t d = 0; d < ns; ++d) {
                        REQUIRE(seg[d].i_from > prev && seg[d].i_from <= seg[d].i_to && seg[d].i_to <= i_to);
                        REQUIRE(seg[d].k_from >= 1 && seg[d].k_from <= seg[d].k_to && seg[d].k_to <= leng);
                        REQUIRE(dom[d].i_from + i_from - 1 == seg[d].i_from && dom[d].ops_begin == at);
                        REQUIRE(ops[at] == 'M');
                        at += dom[d].ops_len;
                        prev = seg[d].i_to;
                    }
                    REQUIRE(at == no);
                    if (ns) {  // a count that is too small is refused, nothing written past it
                        uint32_t small = ns - 1;
                        uint64_t so = no;
                        REQUIRE(msv_spl_sample(gM.data(), gI.data(), gD.data(), rec.data(), m.tsc.data(), m.M, m.b,
                                               m.c, m.j, Lp, 42, 3, i_from, i_to, sample, &small, &so, &trunc,
                                               seg.data(), dom.data(), ops.data()) == MSV_ERR_INVALID_ARGUMENT);
                    }
                }
                // a matrix of zeros: T = 0 at the first draw, every sample truncated and empty
                std::vector<float> z(Le * M, 0.0f);
                std::vector<uint32_t> zr((Le + 1) * 6, 0u);
                uint32_t ns = 9;
                uint64_t no = 9;
                int trunc = 0;
                REQUIRE(msv_spl_sample(z.data(), z.data(), z.data(), zr.data(), m.tsc.data(), m.M, m.b, m.c, m.j, Lp,
                                       42, 3, i_from, i_to, 0, &ns, &no, &trunc, nullptr, nullptr, nullptr) == MSV_OK);
                REQUIRE(trunc == 1 && ns == 0 && no == 0);
            }
        }
    }
    REQUIRE(msv_spl_sample(nullptr, nullptr, nullptr, nullptr, nullptr, 2, 0, 0, 0, 1, 42, 0, 1, 1, 0, nullptr, nullptr,
                           nullptr, nullptr, nullptr, nullptr) == MSV_ERR_INVALID_ARGUMENT);
}

void random_numbers() {
    using namespace msv_host;
    // the key is the envelope's identity: every field moves it, and a draw is 24 bits
    const uint64_t k = spl_key(42, 1, 2, 3, 4);
    REQUIRE(k != spl_key(43, 1, 2, 3, 4) && k != spl_key(42, 2, 2, 3, 4) && k != spl_key(42, 1, 3, 3, 4));
    REQUIRE(k != spl_key(42, 1, 2, 4, 4) && k != spl_key(42, 1, 2, 3, 5) && k == spl_key(42, 1, 2, 3, 4));
    uint64_t sum = 0;
    for (uint32_t d = 0; d < 4096; ++d) {
        const uint32_t u = spl_rand24(k, d);
        REQUIRE(u < (1u << 24));
        sum += u;
    }
    const double mean = static_cast<double>(sum) / 4096.0 / 16777216.0;
    REQUIRE(mean > 0.45 && mean < 0.55);
    // the draw: zero weights are never picked, the top end falls to the last positive weight, T = 0 is refused
    const float w[4] = {0.0f, 0.25f, 0.0f, 0.75f};
    REQUIRE(spl_draw(w, 0) == 1 && spl_draw(w, (1u << 22) - 1) == 1 && spl_draw(w, 1u << 22) == 3);
    REQUIRE(spl_draw(w, (1u << 24) - 1) == 3);
    const float z[2] = {0.0f, 0.0f};
    REQUIRE(spl_draw(z, 5) == -1);
    REQUIRE(spl_scale_down(1.0f, 0) == 1.0f && spl_scale_down(3.0f, 33) == 3.0f * 0x1p-33f);
    REQUIRE(spl_scale_down(1.0f, 130) == 0x1p-130f);
    REQUIRE(spl_scale_down(3.0f, -33) == 3.0f * 0x1p33f && spl_scale_down(0x1p-100f, -150) == 0x1p50f);
}

void clustering(std::mt19937& rng) {
    uint32_t n = 7;
    REQUIRE(msv_spl_cluster(nullptr, 0, 200, nullptr, &n, nullptr) == MSV_OK && n == 0);
    REQUIRE(msv_spl_cluster(nullptr, 0, 0, nullptr, &n, nullptr) == MSV_ERR_INVALID_ARGUMENT);
    std::uniform_int_distribution<uint32_t> jitter(0, 6), where(0, 2);
    std::vector<msv_spl_segment> seg;
    for (int j = 0; j < 600; ++j) {
        const uint32_t base = 1 + 100 * where(rng);
        seg.push_back(msv_spl_segment{base + jitter(rng), base + 60 + jitter(rng), 1 + jitter(rng), 60 + jitter(rng)});
    }
    REQUIRE(msv_spl_cluster(seg.data(), seg.size(), 200, nullptr, &n, nullptr) == MSV_OK);
    REQUIRE(n >= 1 && n <= 3);
    std::vector<msv_spl_envelope> env(n);
    uint32_t n2 = n;
    REQUIRE(msv_spl_cluster(seg.data(), seg.size(), 200, nullptr, &n2, env.data()) == MSV_OK && n2 == n);
    for (uint32_t c = 0; c < n; ++c) {
        REQUIRE(env[c].i_from <= env[c].i_to && env[c].k_from <= env[c].k_to && env[c].count >= 50);
        if (c) REQUIRE(env[c - 1].i_from <= env[c].i_from);
    }
    uint32_t small = n - 1;
    REQUIRE(msv_spl_cluster(seg.data(), seg.size(), 200, nullptr, &small, env.data()) == MSV_ERR_INVALID_ARGUMENT);
    // options: a short struct reads as defaults; a strict one keeps nothing together
    msv_spl_cluster_options o;
    std::memset(&o, 0, sizeof(o));
    o.struct_size = sizeof(uint64_t);
    REQUIRE(msv_spl_cluster(seg.data(), seg.size(), 200, &o, &n2, nullptr) == MSV_OK && n2 == n);
    o.struct_size = sizeof(o);
    o.min_overlap_num = o.min_overlap_den = 1;
    o.max_diagdiff = 1;
    o.min_posterior_num = 0, o.min_posterior_den = 1;
    REQUIRE(msv_spl_cluster(seg.data(), seg.size(), 200, &o, &n2, nullptr) == MSV_OK && n2 > n);
    o.struct_size = 4;
    REQUIRE(msv_spl_cluster(seg.data(), seg.size(), 200, &o, &n2, nullptr) == MSV_ERR_INVALID_ARGUMENT);
    seg[0].i_to = seg[0].i_from - 1;
    REQUIRE(msv_spl_cluster(seg.data(), seg.size(), 200, nullptr, &n2, nullptr) == MSV_ERR_INVALID_ARGUMENT);
}

void region_test_and_workspace() {
    const float begin[6] = {0.5f, 0.0f, 0.0f, 0.5f, 0.0f, 0.0f}, end[6] = {0.0f, 0.0f, 0.5f, 0.0f, 0.0f, 0.5f};
    int multi = -1;
    REQUIRE(msv_dom_is_multidomain(begin, end, 6, 1, 6, 0.5f, &multi) == MSV_OK && multi == 1);
    REQUIRE(msv_dom_is_multidomain(begin, end, 6, 1, 6, 0.75f, &multi) == MSV_OK && multi == 0);
    REQUIRE(msv_dom_is_multidomain(begin, end, 6, 1, 3, 0.25f, &multi) == MSV_OK && multi == 0);
    REQUIRE(msv_dom_is_multidomain(begin, end, 6, 6, 6, 0.25f, &multi) == MSV_OK && multi == 0);
    REQUIRE(msv_dom_is_multidomain(begin, end, 6, 0, 6, 0.25f, &multi) == MSV_ERR_INVALID_ARGUMENT);
    REQUIRE(msv_dom_is_multidomain(begin, end, 6, 4, 3, 0.25f, &multi) == MSV_ERR_INVALID_ARGUMENT);
    REQUIRE(msv_dom_is_multidomain(begin, end, 6, 1, 7, 0.25f, &multi) == MSV_ERR_INVALID_ARGUMENT);

    for (uint32_t S : {2u, 6u, 12u, 22u, 38u})
        for (uint64_t Le : {uint64_t(1), uint64_t(64), uint64_t(129)})
            REQUIRE(msv_spl_item_bytes(S, Le) == 4 * ((Le + 1) * 6 + Le * 3 * S * 64));
    const uint64_t bytes[4] = {msv_spl_item_bytes(2, 10), msv_spl_item_bytes(2, 20), msv_spl_item_bytes(2, 5),
                               msv_spl_item_bytes(2, 20)};
    uint64_t cuts[5], chunks = 0;
    REQUIRE(msv_vit_trace_chunk_cuts(bytes, 4, bytes[1], cuts, &chunks) == MSV_OK && chunks >= 2);
    REQUIRE(msv_vit_trace_chunk_cuts(bytes, 4, bytes[1] - 1, cuts, &chunks) == MSV_ERR_OUT_OF_MEMORY);
}

}  // namespace

int main() {
    std::mt19937 rng(20260414);
    forward_and_samples(rng);
    random_numbers();
    clustering(rng);
    region_test_and_workspace();
    std::printf("sanitize_split passed\n");
    return 0;
}
