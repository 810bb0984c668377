// sanitize_emit.cpp -- the emit stage's host half under AddressSanitizer / UBSan (csrc/Makefile `asan_emit`): the
// fragment decode over every pair index of small models, the tables of a bundled profile and their rejections (a
// group without a total, options out of range), the definition by slices (a first above 2^32, n = 0), both modes and
// insert modes, every truncation length of a short walk, the structure of every truth and the score of each true
// path with its rejections.  Host-only sources, its own main.
#include <unistd.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "emit_host.h"
#include "msv.h"

namespace {

#define REQUIRE(cond)                                                        \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                    \
        }                                                                    \
    } while (0)

struct Result {
    std::vector<uint8_t> codes, ops, truncated;
    std::vector<uint64_t> offsets, domain_offsets;
    std::vector<msv_vit_domain> domains;
};

Result generate(const msv_hmm* hmm, const msv_emit_options* o, uint64_t seed, uint64_t first, uint64_t n) {
    msv_emit_result* r = nullptr;
    REQUIRE(msv_emit_generate(hmm, o, seed, first, n, &r) == MSV_OK);
    Result out;
    REQUIRE(msv_emit_result_count(r) == n && msv_emit_result_chunks(r) == 0);
    out.codes.resize(msv_emit_result_residues(r));
    out.ops.resize(msv_emit_result_ops(r));
    out.domains.resize(msv_emit_result_domains(r));
    out.truncated.resize(n);
    out.offsets.resize(n + 1);
    out.domain_offsets.resize(n + 1);
    REQUIRE(msv_emit_result_copy(r, out.codes.data(), out.offsets.data(), out.domain_offsets.data(),
                                 out.domains.data(), out.ops.data(), out.truncated.data()) == MSV_OK);
    msv_emit_result_free(r);
    return out;
}

msv_emit_options options(uint64_t Lc, bool unihit, int insert_mode, uint64_t max_length) {
    msv_emit_options o;
    std::memset(&o, 0, sizeof(o));
    o.struct_size = sizeof(o);
    o.length = Lc;
    o.length_set = 1;
    o.unihit = unihit ? 1 : 0;
    o.insert_mode = insert_mode;
    o.max_length = max_length;
    return o;
}

// Every truth replays, its domains are disjoint and in order, and every k lies in the model.
void structure(const Result& r, uint32_t leng, uint64_t max_length, bool unihit) {
    const uint64_t n = r.truncated.size();
    REQUIRE(r.offsets[0] == 0 && r.domain_offsets[0] == 0);
    uint64_t ops_at = 0;
    for (uint64_t q = 0; q < n; ++q) {
        const uint64_t L = r.offsets[q + 1] - r.offsets[q];
        REQUIRE(L <= max_length && (r.truncated[q] != 0) == (L == max_length));
        uint64_t last = 0;
        const uint64_t nd = r.domain_offsets[q + 1] - r.domain_offsets[q];
        if (unihit && !r.truncated[q]) REQUIRE(nd == 1);
        for (uint64_t x = r.domain_offsets[q]; x < r.domain_offsets[q + 1]; ++x) {
            const msv_vit_domain& d = r.domains[x];
            REQUIRE(d.seq == q && d.ops_begin == ops_at && d.i_from > last && d.i_from <= d.i_to && d.i_to <= L);
            REQUIRE(d.k_from >= 1 && d.k_from <= d.k_to && d.k_to <= leng && d.ops_len >= 1);
            uint64_t i = d.i_from - 1, k = d.k_from - 1;
            for (uint32_t j = 0; j < d.ops_len; ++j) {
                const uint8_t op = r.ops[d.ops_begin + j];
                REQUIRE(op == 'M' || op == 'I' || op == 'D');
                i += op != 'D';
                k += op != 'I';
            }
            REQUIRE(i == d.i_to && k == d.k_to && r.ops[d.ops_begin] == 'M');
            const bool cut = r.truncated[q] && x + 1 == r.domain_offsets[q + 1] && d.i_to == L;
            if (!cut) REQUIRE(r.ops[d.ops_begin + d.ops_len - 1] != 'I');
            ops_at += d.ops_len;
            last = d.i_to;
        }
        for (uint64_t i = r.offsets[q]; i < r.offsets[q + 1]; ++i) REQUIRE(r.codes[i] < 20);
    }
    REQUIRE(ops_at == r.ops.size() && r.offsets[n] == r.codes.size() && r.domain_offsets[n] == r.domains.size());
}

void fragments() {
    for (uint32_t leng : {1u, 2u, 3u, 7u, 64u, 65u}) {
        uint32_t idx = 0;
        for (uint32_t s = 1; s <= leng; ++s)
            for (uint32_t e = s; e <= leng; ++e, ++idx) {
                uint32_t ks = 0, ke = 0;
                msv_host::emit_fragment(idx, leng, &ks, &ke);
                REQUIRE(ks == s && ke == e);
            }
        REQUIRE(idx == leng * (leng + 1) / 2);
    }
    uint32_t ks = 0, ke = 0;
    msv_host::emit_fragment(65535u * 65536u / 2 - 1, 65535, &ks, &ke);
    REQUIRE(ks == 65535 && ke == 65535);
}

void bundled(const std::string& root) {
    msv_hmm* hmm = nullptr;
    REQUIRE(msv_hmm_read((root + "/data/profile_HMMs/100.hmm").c_str(), &hmm) == MSV_OK);
    const uint32_t M = static_cast<uint32_t>(msv_hmm_model_length(hmm)), leng = M - 1;
    std::vector<uint32_t> bg(19), match(M * 19), insert(M * 19), trans(M * 4), sp(2);
    msv_emit_options o = options(400, false, MSV_INSERTS_LOG_ODDS, 0);
    REQUIRE(msv_emit_tables(hmm, &o, bg.data(), match.data(), insert.data(), trans.data(), sp.data()) == MSV_OK);
    REQUIRE(msv_emit_tables(hmm, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == MSV_OK);
    REQUIRE(msv_emit_tables(nullptr, &o, nullptr, nullptr, nullptr, nullptr, nullptr) == MSV_ERR_INVALID_ARGUMENT);
    REQUIRE(sp[0] == static_cast<uint32_t>(std::floor(16777216.0 * 400.0 / 403.0)) && sp[1] == (1u << 23));
    for (uint32_t k = 1; k <= leng; ++k)
        for (int j = 1; j < 19; ++j)
            REQUIRE(match[k * 19 + j] >= match[k * 19 + j - 1] && match[k * 19 + j] <= (1u << 24));
    for (uint32_t k = 1; k < leng; ++k) REQUIRE(trans[k * 4] <= trans[k * 4 + 1] && trans[k * 4 + 1] <= (1u << 24));
    for (int j = 0; j < 4; ++j) REQUIRE(trans[j] == 0 && trans[leng * 4 + j] == 0);
    msv_emit_options bad = o;
    bad.unihit = 2;
    REQUIRE(msv_emit_tables(hmm, &bad, nullptr, nullptr, nullptr, nullptr, nullptr) == MSV_ERR_INVALID_ARGUMENT);
    bad = o;
    bad.max_length = 1ull << 31;
    REQUIRE(msv_emit_tables(hmm, &bad, nullptr, nullptr, nullptr, nullptr, nullptr) == MSV_ERR_INVALID_ARGUMENT);
    bad = o;
    bad.insert_mode = 7;
    REQUIRE(msv_emit_tables(hmm, &bad, nullptr, nullptr, nullptr, nullptr, nullptr) == MSV_ERR_INVALID_ARGUMENT);
    bad = o;
    bad.struct_size = 4;
    REQUIRE(msv_emit_tables(hmm, &bad, nullptr, nullptr, nullptr, nullptr, nullptr) == MSV_ERR_INVALID_ARGUMENT);
    uint32_t unihit_sp[2];
    msv_emit_options uni = options(0, true, MSV_INSERTS_ZERO, 0);
    REQUIRE(msv_emit_tables(hmm, &uni, nullptr, nullptr, insert.data(), nullptr, unihit_sp) == MSV_OK);
    REQUIRE(unihit_sp[0] == 0 && unihit_sp[1] == 0);
    for (int j = 0; j < 19; ++j) REQUIRE(insert[19 + j] == bg[j]);

    std::vector<float> msc(20 * M), isc(20 * M), tsc(7 * M);
    float b = 0, c = 0, j = 0;
    REQUIRE(msv_hmm_viterbi_scores(hmm, MSV_INSERTS_LOG_ODDS, msc.data(), isc.data(), tsc.data(), &b, &c, &j) ==
            MSV_OK);

    for (int mode = 0; mode < 4; ++mode) {
        const bool unihit = mode & 1;
        const int ins = mode & 2 ? MSV_INSERTS_LOG_ODDS : MSV_INSERTS_ZERO;
        for (uint64_t Lc : {0ull, 1ull, 400ull}) {
            msv_emit_options w = options(Lc, unihit, ins, 0);
            for (uint64_t first : {0ull, (1ull << 32) + 77ull}) {
                const Result whole = generate(hmm, &w, 42, first, 40), part = generate(hmm, &w, 42, first + 30, 7);
                structure(whole, leng, 1ull << 20, unihit);
                const uint64_t c0 = whole.offsets[30], c1 = whole.offsets[37];
                REQUIRE(part.codes.size() == c1 - c0);
                REQUIRE(std::memcmp(part.codes.data(), whole.codes.data() + c0, c1 - c0) == 0);
                for (uint64_t q = 0; q <= 7; ++q) REQUIRE(part.offsets[q] == whole.offsets[30 + q] - c0);
                const uint64_t d0 = whole.domain_offsets[30];
                REQUIRE(part.domains.size() == whole.domain_offsets[37] - d0);
                for (uint64_t x = 0; x < part.domains.size(); ++x) {
                    const msv_vit_domain &p = part.domains[x], &q = whole.domains[d0 + x];
                    REQUIRE(p.i_from == q.i_from && p.i_to == q.i_to && p.k_from == q.k_from && p.k_to == q.k_to &&
                            p.ops_len == q.ops_len && p.seq + 30 == q.seq);
                    REQUIRE(std::memcmp(&part.ops[p.ops_begin], &whole.ops[q.ops_begin], p.ops_len) == 0);
                }
                // the score of every true path is finite, and below it nothing is accepted that does not replay
                for (uint64_t q = 0; q < 40; ++q) {
                    const uint64_t L = whole.offsets[q + 1] - whole.offsets[q];
                    const uint32_t nd = static_cast<uint32_t>(whole.domain_offsets[q + 1] - whole.domain_offsets[q]);
                    double sc = 0;
                    REQUIRE(msv_emit_path_score(msc.data(), ins ? isc.data() : nullptr, tsc.data(), M, b, c, j,
                                                whole.codes.data() + whole.offsets[q], L,
                                                whole.domains.data() + whole.domain_offsets[q], nd, whole.ops.data(),
                                                &sc) == MSV_OK);
                    REQUIRE(std::isfinite(sc) && sc < 1e6);
                    msv_vit_domain wrong = whole.domains[whole.domain_offsets[q]];
                    wrong.k_to += 1;
                    REQUIRE(msv_emit_path_score(msc.data(), nullptr, tsc.data(), M, b, c, j,
                                                whole.codes.data() + whole.offsets[q], L, &wrong, 1, whole.ops.data(),
                                                &sc) == MSV_ERR_INVALID_ARGUMENT);
                }
            }
            const Result other = generate(hmm, &w, 43, 0, 8), same = generate(hmm, &w, 42, 0, 8);
            REQUIRE(other.codes != same.codes);
        }
    }
    // every truncation length of short walks, in a domain and outside one
    for (uint64_t cut = 1; cut <= 40; ++cut) {
        msv_emit_options w = options(3, false, MSV_INSERTS_ZERO, cut);
        const Result r = generate(hmm, &w, 7, 0, 64);
        structure(r, leng, cut, false);
    }
    double sc = 0;
    REQUIRE(msv_emit_path_score(msc.data(), nullptr, tsc.data(), M, b, c, j, nullptr, 0, nullptr, 0, nullptr, &sc) ==
                MSV_OK &&
            std::isinf(sc) && sc < 0);
    const Result none = generate(hmm, &o, 1, 0, 0);
    REQUIRE(none.offsets.size() == 1 && none.codes.empty());
    msv_emit_result* r = nullptr;
    REQUIRE(msv_emit_generate(hmm, &o, 1, 0, 1ull << 32, &r) == MSV_ERR_INVALID_ARGUMENT && r == nullptr);
    REQUIRE(msv_emit_result_copy(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) ==
            MSV_ERR_INVALID_ARGUMENT);
    msv_emit_result_free(nullptr);
    REQUIRE(msv_emit_workspace_bytes(3, 17, 2, 5, 1) == 48 + 32 + 32 + 16 + 32 + 64 + 16);
    REQUIRE(msv_emit_workspace_bytes(3, 17, 2, 5, 0) == 48 + 32 + 32);
    msv_hmm_destroy(hmm);
}

// A LENG-2 profile whose node 1 has the given transition line: a group without a total is refused.
void rejected(const char* transitions, msv_status want) {
    char path[] = "/tmp/sanitize_emit_XXXXXX";
    const int fd = mkstemp(path);
    REQUIRE(fd >= 0);
    std::string text =
        "HMMER3/b [sanitize_emit]\nNAME  tiny\nLENG  2\nALPH  amino\n"
        "STATS LOCAL MSV       -9.9000  0.70000\nSTATS LOCAL VITERBI  -10.5000  0.70000\n"
        "STATS LOCAL FORWARD   -4.0000  0.70000\nHMM          A        C        D        E        F        G        H"
        "        I        K        L        M        N        P        Q        R        S        T        V        W"
        "        Y   \n            m->m     m->i     m->d     i->m     i->i     d->m     d->d\n";
    std::string row;
    for (int x = 0; x < 20; ++x) row += "  2.99573";
    text += "  COMPO " + row + "\n        " + row +
            "\n          0.05000  4.10000  3.00000  0.62000  0.77000  0.00000        *\n";
    text += "      1 " + row + "\n        " + row + "\n        " + transitions + "\n";
    text += "      2 " + row + "\n        " + row +
            "\n          0.05000  4.10000        *  0.62000  0.77000  0.00000        *\n//\n";
    REQUIRE(write(fd, text.data(), text.size()) == static_cast<ssize_t>(text.size()));
    close(fd);
    msv_hmm* hmm = nullptr;
    REQUIRE(msv_hmm_read(path, &hmm) == MSV_OK);
    REQUIRE(msv_hmm_model_length(hmm) == 3);
    REQUIRE(msv_emit_tables(hmm, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == want);
    if (want == MSV_OK) {
        msv_emit_options w = options(0, true, MSV_INSERTS_ZERO, 0);
        structure(generate(hmm, &w, 3, 0, 200), 2, 1ull << 20, true);
    }
    msv_hmm_destroy(hmm);
    unlink(path);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) {
        std::fprintf(stderr, "usage: %s <repository root>\n", argv[0]);
        return 2;
    }
    fragments();
    bundled(argv[1]);
    rejected("  0.22314  2.30259  2.30259  0.69315  0.69315  0.69315  0.69315", MSV_OK);
    rejected("  0.22314  2.30259  2.30259  0.69315  0.69315  200.0000  200.0000", MSV_ERR_INVALID_ARGUMENT);  // D
    rejected("  200.0000  200.0000  200.0000  0.69315  0.69315  0.69315  0.69315", MSV_ERR_INVALID_ARGUMENT);  // M
    rejected("  0.22314  2.30259  2.30259  200.0000  200.0000  0.69315  0.69315", MSV_ERR_INVALID_ARGUMENT);  // I
    std::printf("sanitize_emit passed\n");
    return 0;
}
