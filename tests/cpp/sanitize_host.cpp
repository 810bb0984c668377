// sanitize_host.cpp -- host-only driver for the sanitizer builds (csrc/Makefile `asan`, `tsan`).
//
// Exercises every host translation unit with no GPU: the .hmm parser (all 24 profiles, truncated
// files, a last line without its newline -- the reference's remove_prefix(npos) site,
// Profile_HMM.cpp:10-11), the FASTA reader (the golden edge cases, first-line / EOF cases -- the
// reference's sequences.back() on an empty vector, FASTA_protein_sequences.cpp:22 -- and a file large
// enough for the multi-threaded chunked path), the precompute (MSV_HMM.cpp:35-57) and the CPU DP
// (MSV_HMM.cpp:74-113) against the golden scores, msv_shard_bounds, the Viterbi stage's table builder
// and CPU DP (msv_hmm_viterbi_scores, msv_vit_cpu_score), and the kernel-layout tables the device layer
// uploads (table_layout.cpp: every MSV, cooperative and Viterbi layout, at exact-fit model lengths), and the MSV
// plan policy (msv_plan.cpp) against the plans recorded on the device (tests/golden/msv_plans.json), with the host
// calls' part of it: rebase_offsets, plan_call's mode and staging layout, the multi-device chunk cuts.
// Usage: sanitize_host <repo_root>
#include <dirent.h>
#include <unistd.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <initializer_list>
#include <limits>
#include <map>
#include <random>
#include <sstream>
#include <string>
#include <vector>

#include "host_cpu.h"
#include "msv.h"
#include "msv_hmm.hpp"
#include "msv_plan.h"

static int failures = 0;
#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) {                                                           \
            std::printf("sanitize_host: FAILED %s (line %d)\n", #c, __LINE__); \
            ++failures;                                                       \
        }                                                                     \
    } while (0)

static std::string slurp(const std::string& path) {
    std::ifstream f(path, std::ios::binary);
    std::stringstream ss;
    ss << f.rdbuf();
    return ss.str();
}

static void spit(const std::string& path, const std::string& text) {
    std::ofstream f(path, std::ios::binary);
    f << text;
}

struct Table {
    std::vector<float> e;
    size_t M = 0;
    float bmk = 0, ec = 0, ej = 0;
};

static bool load_table(const std::string& path, Table& t) {
    msv_hmm* h = nullptr;
    if (msv_hmm_read(path.c_str(), &h) != MSV_OK) return false;
    t.M = msv_hmm_model_length(h);
    t.e.assign(20 * t.M, 0.f);
    const bool ok = msv_hmm_msv_scores(h, t.e.data(), &t.bmk, &t.ec, &t.ej) == MSV_OK;
    msv_hmm_destroy(h);
    return ok;
}

static float score(const Table& t, const uint8_t* codes, size_t L) {
    return msv_host::run_on_sequence(t.e.data(), t.M, t.bmk, t.ec, t.ej, codes, L);
}

static uint32_t bits(float x) {
    uint32_t u;
    std::memcpy(&u, &x, 4);
    return u;
}

// tests/golden/<file>.tsv: profile, seq, length, score (hex), score
static std::map<std::pair<std::string, int>, float> golden(const std::string& path) {
    std::map<std::pair<std::string, int>, float> g;
    std::ifstream f(path);
    std::string line;
    while (std::getline(f, line)) {
        if (line.empty() || line[0] == '#') continue;
        std::istringstream ss(line);
        std::string prof, hex;
        int seq;
        size_t len;
        ss >> prof >> seq >> len >> hex;
        g[{prof, seq}] = static_cast<float>(std::strtod(hex.c_str(), nullptr));
    }
    return g;
}

static void check_scores(const std::string& root, const std::string& fasta, const std::string& gold,
                         const std::vector<std::string>& profiles) {
    msv_fasta* f = nullptr;
    CHECK(msv_fasta_read((root + "/data/FASTA_files/" + fasta).c_str(), &f) == MSV_OK);
    if (!f) return;
    const auto g = golden(root + "/tests/golden/" + gold);
    size_t checked = 0;
    for (const auto& name : profiles) {
        Table t;
        CHECK(load_table(root + "/data/profile_HMMs/" + name, t));
        for (size_t s = 0; s < msv_fasta_count(f); ++s) {
            const uint64_t* o = msv_fasta_offsets(f);
            const float got = score(t, msv_fasta_codes(f) + o[s], o[s + 1] - o[s]);
            const auto it = g.find({name, static_cast<int>(s)});
            CHECK(it != g.end());
            if (it != g.end()) {
                if (bits(got) != bits(it->second))
                    std::printf("  %s seq %zu: %a vs golden %a\n", name.c_str(), s, got, it->second);
                CHECK(bits(got) == bits(it->second));
                ++checked;
            }
        }
    }
    msv_fasta_destroy(f);
    std::printf("  %s: %zu scores bitwise equal to %s\n", fasta.c_str(), checked, gold.c_str());
}

struct Parsed {
    msv_status status;
    std::vector<uint64_t> lengths;
    std::string codes;
    size_t rejected = 0;
};

static Parsed parse_text(const std::string& dir, const std::string& name, const std::string& text) {
    const std::string path = dir + "/" + name;
    spit(path, text);
    Parsed p;
    msv_fasta* f = nullptr;
    p.status = msv_fasta_read(path.c_str(), &f);
    if (p.status == MSV_OK) {
        const uint64_t* o = msv_fasta_offsets(f);
        for (size_t s = 0; s < msv_fasta_count(f); ++s) p.lengths.push_back(o[s + 1] - o[s]);
        p.codes.assign(reinterpret_cast<const char*>(msv_fasta_codes(f)), o[msv_fasta_count(f)]);
        p.rejected = msv_fasta_rejected(f);
        msv_fasta_destroy(f);
    }
    std::remove(path.c_str());
    return p;
}

// ---- kernel-layout tables (table_layout.cpp) ----
// The expected table is built the other way round from the builders: they walk the table's slots and ask
// which state belongs there; here every state 1..R is PLACED at the index its layout comment gives, in a
// table that is otherwise -inf (rows 0-19) and +inf (the poison row), and the two are compared bit for bit.
// Entry (r, j) of the synthetic score table is the exactly representable r * 4096 + j: no two states share
// a value.  The tables are heap vectors of exactly 20 x model_length, so a read past either end is ASan's.
static const float kNinf = -std::numeric_limits<float>::infinity();
static const float kPinf = std::numeric_limits<float>::infinity();

static std::vector<float> synthetic(uint32_t model_length, float base = 0.0f) {
    std::vector<float> es(20 * static_cast<size_t>(model_length));
    for (uint32_t r = 0; r < 20; ++r)
        for (uint32_t j = 0; j < model_length; ++j)
            es[r * static_cast<size_t>(model_length) + j] = base + r * 4096.0f + j;
    return es;
}

static void same_tables(const char* what, int a, int b, int c, uint32_t R, const std::vector<float>& got,
                        const std::vector<float>& want) {
    const bool same = got.size() == want.size() &&
                      (want.empty() || std::memcmp(got.data(), want.data(), want.size() * 4) == 0);
    if (!same) std::printf("  %s (%d, %d, %d) R = %u: size %zu vs %zu\n", what, a, b, c, R, got.size(), want.size());
    CHECK(same);
}

// [21][S/4][G] float4; split: A [20][sa/4][G] float4, then B [21][G][HBP] float2 (HBP = (S - sa)/2 rounded up to even)
static void check_variant_layout(int G, int S, int sa) {
    const uint32_t cap = static_cast<uint32_t>(G * S);
    for (uint32_t R : {cap, cap - 1, 1u}) {
        const uint32_t M = R + 1;
        const std::vector<float> es = synthetic(M);
        const size_t SA = sa ? sa : S, a_rows = sa ? 20 : 21, a_size = a_rows * (SA / 4) * G * 4;
        const size_t HB = sa ? (S - sa) / 2 : 0, HBP = (HB + 1) & ~size_t(1), b_size = sa ? 21 * G * HBP * 2 : 0;
        std::vector<float> want(a_size + b_size, kNinf);
        if (!sa) std::fill(want.begin() + 20 * (SA / 4) * G * 4, want.begin() + a_size, kPinf);
        std::fill(want.begin() + a_size + 20 * G * HBP * 2, want.end(), kPinf);
        for (size_t r = 0; r < 20; ++r)
            for (uint32_t j = 1; j <= R; ++j) {
                const size_t gl = (j - 1) / S, w = (j - 1) % S;
                const size_t at = w < SA ? ((r * (SA / 4) + w / 4) * G + gl) * 4 + w % 4
                                         : a_size + ((r * G + gl) * HBP + (w - SA) / 2) * 2 + (w - SA) % 2;
                want[at] = r * 4096.0f + j;
            }
        same_tables("msv_variant_table", G, S, sa, R, msv_host::msv_variant_table(es.data(), M, G, S, sa), want);
    }
}

// [21][W][sa/2][64] float2, then (sa < S) [21][W][64][S - sa] floats; wave w's slot (l, k) is state
// w (64 S - halo) - halo + l S + k + 1, so the first `halo` states of wave w > 0 repeat wave w-1's last ones
static void check_coop_layout(int W, int S, int sa) {
    const int halo = (16 + S - 1) / S * S;  // msv_coop.hip's variants
    const uint32_t cap = static_cast<uint32_t>(W * (64 * S - halo));
    for (uint32_t R : {cap, cap - 1, 1u}) {
        const uint32_t M = R + 1;
        const std::vector<float> es = synthetic(M);
        const size_t H = sa / 2, SB = S - sa, a_size = size_t(21) * W * H * 64 * 2, b_size = size_t(21) * W * 64 * SB;
        std::vector<float> want(a_size + b_size, kNinf);
        std::fill(want.begin() + size_t(20) * W * H * 64 * 2, want.begin() + a_size, kPinf);
        std::fill(want.begin() + a_size + size_t(20) * W * 64 * SB, want.end(), kPinf);
        size_t placed = 0;
        for (size_t r = 0; r < 20; ++r)
            for (uint32_t j = 1; j <= R; ++j)
                for (int w = 0; w < W; ++w) {
                    const int64_t local = int64_t(j) - 1 + halo - int64_t(w) * (64 * S - halo);  // slot within wave w
                    if (local < 0 || local >= 64 * S) continue;
                    const size_t l = local / S, k = local % S;
                    const size_t at = k < size_t(sa) ? (((r * W + w) * H + k / 2) * 64 + l) * 2 + k % 2
                                                     : a_size + ((r * W + w) * 64 + l) * SB + (k - sa);
                    want[at] = r * 4096.0f + j;
                    ++placed;
                }
        CHECK(placed >= 20 * size_t(R));  // every state in at least one wave
        same_tables("msv_coop_table", W, S, sa, R, msv_host::msv_coop_table(es.data(), M, W, S, sa, halo), want);
    }
}

// et / it [20][C2][64 team] float2, tt [7][C2][64 team] float2, C2 = (S + 1) / 2: state k = l S + q + 1 is half
// q % 2 of chunk q / 2 of lane l.  Slot arrays (vit_kernel.h): MM_IN IM_IN DM_IN MI II MD_IN DD_IN, from the file
// order m->m m->i m->d i->m i->i d->m d->d of node k-1 (the _IN ones, k >= 2) or node k (MI, II, k < K).
static void check_vit_layout(int S, int team, bool isc) {
    const uint32_t cap = static_cast<uint32_t>(64 * S * team);
    for (uint32_t K : {cap, cap - 1, 1u}) {
        const uint32_t M = K + 1;
        const std::vector<float> msc = synthetic(M), ins = synthetic(M, 100000.0f);
        std::vector<float> tsc(7 * static_cast<size_t>(M));
        for (size_t i = 0; i < tsc.size(); ++i) tsc[i] = -static_cast<float>(i + 1);
        const size_t C2 = (S + 1) / 2, L = size_t(64) * team, rows = C2 * L * 2;
        std::vector<float> et(20 * rows, kNinf), it(isc ? 20 * rows : 0, 0.0f), tt(7 * rows, kNinf);
        static const int from_prev[7] = {0, 3, 5, -1, -1, 2, 6}, from_self[7] = {-1, -1, -1, 1, 4, -1, -1};
        for (uint32_t k = 1; k <= K; ++k) {
            const size_t l = (k - 1) / S, q = (k - 1) % S, at = ((q / 2) * L + l) * 2 + q % 2;
            for (size_t r = 0; r < 20; ++r) {
                et[r * rows + at] = r * 4096.0f + k;
                if (isc && k < K) it[r * rows + at] = 100000.0f + r * 4096.0f + k;
            }
            for (size_t j = 0; j < 7; ++j) {
                if (from_prev[j] >= 0 && k >= 2) tt[j * rows + at] = tsc[(k - 1) * size_t(7) + from_prev[j]];
                if (from_self[j] >= 0 && k < K) tt[j * rows + at] = tsc[k * size_t(7) + from_self[j]];
            }
        }
        const msv_host::VitTables t =
            msv_host::vit_tables(msc.data(), isc ? ins.data() : nullptr, tsc.data(), M, S, team, isc);
        same_tables("vit_tables et", S, team, isc, K, t.et, et);
        same_tables("vit_tables it", S, team, isc, K, t.it, it);
        same_tables("vit_tables tt", S, team, isc, K, t.tt, tt);
    }
}

static void check_layouts() {
    // (G, S) and (G, S, sa) of the generated variant lists, (waves, S, sa) of msv_coop.hip's, (S, team) of the
    // Viterbi families (vit_w2_s13_ga4, vit_w2_s12_ga4, vit_w1_s22_ea / vit_s22_t0gi)
    check_variant_layout(4, 28, 0);
    check_variant_layout(16, 8, 0);
    check_variant_layout(64, 24, 0);
    check_variant_layout(32, 62, 60);  // HB = 1: the padded half
    check_variant_layout(64, 34, 32);
    check_coop_layout(4, 2, 2);
    check_coop_layout(4, 6, 6);
    check_coop_layout(4, 8, 6);
    check_coop_layout(4, 10, 6);
    for (bool isc : {false, true}) {
        check_vit_layout(13, 2, isc);
        check_vit_layout(12, 2, isc);
        check_vit_layout(22, 1, isc);
    }
    std::printf("  table layouts: 5 MSV, 4 cooperative and 3 Viterbi geometries at 3 model lengths each\n");
}

// ---- the MSV plan policy (msv_plan.cpp) ----
// The shape tables come from the lists the kernel tables are built from, under macros of this file: index i
// here is index i of msvk::variants() / msvk::coop_variants(), and the names are the kernels' names.
struct NamedVariant {
    msvplan::VariantShape shape;
    const char* name;
};
struct NamedCoop {
    msvplan::CoopShape shape;
    const char* name;
};
// msv_kernel.h: lds_rows_for(G, S) < kTableRows, the table does not fit the 160 KiB of LDS
static constexpr bool big_table(int G, int S) { return 163840 / (G * S * 4) < 21; }
// (the grid kernel exists for the one-sequence-per-wave variants: msv_kernel_impl.h grid_fn)
#define MSV_VARIANT(G, S, W, P, D) \
    NamedVariant{{G, S, W, P, D, 0, big_table(G, S), G == 64 && D == 1}, "msv_g" #G "_s" #S "_w" #W "_p" #P "_d" #D}
#define MSV_SPLIT_VARIANT(G, S, SA, W, P) \
    NamedVariant{{G, S, W, P, 1, SA, false, G == 64}, "msv_g" #G "_s" #S "_a" #SA "_w" #W "_p" #P "_d1"}
#define MSV_COOP_VARIANT(W, S) NamedCoop{{W, S, (16 + S - 1) / S * S, S, true}, "msv_coop_w" #W "_s" #S}
#define MSV_COOP_SPLIT_VARIANT(W, S, SA) \
    NamedCoop{{W, S, (16 + S - 1) / S * S, SA, true}, "msv_coop_w" #W "_s" #S "_a" #SA}
static const NamedVariant kVariants[] = {
#include "msv_variants_0.inc"
#include "msv_variants_1.inc"
#include "msv_variants_2.inc"
#include "msv_variants_3.inc"
#include "msv_variants_4.inc"
#include "msv_variants_5.inc"
#include "msv_variants_6.inc"
#include "msv_variants_7.inc"
};
static const NamedCoop kCoopVariants[] = {
#include "msv_coop_variants.inc"
};

static msvplan::Tables plan_tables() {
    msvplan::Tables t;
    for (const NamedVariant& v : kVariants) t.variants.push_back(v.shape);
    for (const NamedCoop& c : kCoopVariants) t.coop.push_back(c.shape);
    return t;
}

static int variant_index(const std::string& name) {
    for (size_t i = 0; i < sizeof(kVariants) / sizeof(kVariants[0]); ++i)
        if (name == kVariants[i].name) return static_cast<int>(i);
    return -1;
}

static std::string plan_name(const msvplan::PlanSet& ps, msvplan::Kind kind) {
    const int i = kind == msvplan::kCoop ? ps.coop : kind == msvplan::kLatency ? ps.lat : kind == msvplan::kMid ? ps.mid : ps.main;
    if (i < 0) return "";
    return kind == msvplan::kCoop ? kCoopVariants[i].name : kVariants[i].name;
}

// A JSON value of tests/golden/msv_plans.json: objects, arrays, strings without escapes, unsigned integers.
struct Json {
    std::map<std::string, Json> object;
    std::vector<Json> array;
    std::string string;
    uint64_t number = 0;
    const Json& operator[](const char* key) const {
        static const Json none;
        const auto it = object.find(key);
        return it == object.end() ? none : it->second;
    }
};

static bool parse_json(const std::string& text, size_t& at, Json& out) {
    auto skip = [&] {
        while (at < text.size() && std::strchr(" \t\r\n,:", text[at])) ++at;
    };
    skip();
    if (at >= text.size()) return false;
    if (text[at] == '"') {
        const size_t end = text.find('"', at + 1);
        if (end == std::string::npos) return false;
        out.string = text.substr(at + 1, end - at - 1);
        at = end + 1;
        return true;
    }
    if (text[at] == '{' || text[at] == '[') {
        const bool object = text[at++] == '{';
        for (skip(); at < text.size() && text[at] != (object ? '}' : ']'); skip()) {
            Json key, value;
            if (object && (!parse_json(text, at, key) || key.string.empty())) return false;
            if (!parse_json(text, at, value)) return false;
            if (object) out.object[key.string] = value;
            else out.array.push_back(value);
        }
        return at++ < text.size();
    }
    const size_t start = at;
    while (at < text.size() && text[at] >= '0' && text[at] <= '9') out.number = out.number * 10 + (text[at++] - '0');
    return at > start;
}

static const char* const kPlanKeys[4][3] = {{"variant", "blocks", ""},
                                            {"latency_variant", "latency_blocks", "latency_max_n"},
                                            {"mid_variant", "mid_blocks", "mid_max_n"},
                                            {"coop_variant", "coop_blocks", "coop_max_n"}};

// 9a. choose() and which() give every recorded profile its recorded plans, ranges and variant_for(n), with the
// recorded CU count and grids; then every model length 1..4096 (4097: none) keeps the policy's invariants.
static void check_recorded_plans(const std::string& root, const msvplan::Tables& tables) {
    Json rec;
    size_t at = 0;
    const std::string text = slurp(root + "/tests/golden/msv_plans.json");
    CHECK(parse_json(text, at, rec));
    const int cus = static_cast<int>(rec["cus"].number);
    CHECK(cus > 0 && rec["records"].array.size() >= 100);
    std::map<std::string, int> recorded_blocks;  // a kernel's persistent grid on the recorded device
    for (const Json& r : rec["records"].array)
        for (const auto& keys : kPlanKeys)
            if (!r["describe"][keys[0]].string.empty())
                recorded_blocks[r["describe"][keys[0]].string] = static_cast<int>(r["describe"][keys[1]].number);
    bool asked_mid = false;
    const msvplan::BlocksOf blocks_of = [&](msvplan::Kind kind, int i) {
        asked_mid |= kind == msvplan::kMid;
        const auto it = recorded_blocks.find(kind == msvplan::kCoop ? kCoopVariants[i].name : kVariants[i].name);
        return it == recorded_blocks.end() ? cus : it->second;  // unrecorded: one block per CU
    };
    size_t points = 0;
    for (const Json& r : rec["records"].array) {
        const uint32_t states = static_cast<uint32_t>(r["states"].number);
        const std::string& forced = r["forced"].string;
        CHECK(forced.empty() || variant_index(forced) >= 0);
        const msvplan::PlanSet ps = msvplan::choose(tables, states, true, variant_index(forced), cus, blocks_of);
        const Json& d = r["describe"];
        const bool same = plan_name(ps, msvplan::kMain) == d["variant"].string &&
                          plan_name(ps, msvplan::kLatency) == d["latency_variant"].string &&
                          plan_name(ps, msvplan::kMid) == d["mid_variant"].string &&
                          plan_name(ps, msvplan::kCoop) == d["coop_variant"].string &&
                          ps.lat_max_n == d["latency_max_n"].number && ps.mid_max_n == d["mid_max_n"].number &&
                          ps.coop_max_n == d["coop_max_n"].number;
        if (!same)
            std::printf("  %u states %s: chose %s / %s <= %llu / %s <= %llu / %s <= %llu\n", states, forced.c_str(),
                        plan_name(ps, msvplan::kMain).c_str(), plan_name(ps, msvplan::kLatency).c_str(),
                        static_cast<unsigned long long>(ps.lat_max_n), plan_name(ps, msvplan::kMid).c_str(),
                        static_cast<unsigned long long>(ps.mid_max_n), plan_name(ps, msvplan::kCoop).c_str(),
                        static_cast<unsigned long long>(ps.coop_max_n));
        CHECK(same);
        CHECK(r["variant_for"].array.size() >= 3);
        for (const Json& point : r["variant_for"].array) {
            CHECK(point.array.size() == 2);
            if (point.array.size() != 2) continue;
            const uint64_t n = point.array[0].number;
            const std::string got = plan_name(ps, msvplan::which(ps, n, true, false));
            if (got != point.array[1].string)
                std::printf("  %u states %s, n = %llu: %s, recorded %s\n", states, forced.c_str(),
                            static_cast<unsigned long long>(n), got.c_str(), point.array[1].string.c_str());
            CHECK(got == point.array[1].string);
            CHECK(msvplan::which(ps, n, false, false) == msvplan::kMain);
            ++points;
        }
    }
    for (uint32_t states = 1; states <= 4096; ++states)
        for (bool same_EJ : {true, false}) {
            const msvplan::PlanSet ps = msvplan::choose(tables, states, same_EJ, -1, cus, blocks_of);
            CHECK(ps.main >= 0);
            if (ps.main < 0) continue;
            for (int i : {ps.main, ps.lat, ps.mid})
                CHECK(i < 0 || static_cast<uint32_t>(tables.variants[i].states()) >= states);
            int smallest = -1;  // the covering cooperative variant of the fewest states
            for (size_t i = 0; i < tables.coop.size(); ++i)
                if (static_cast<uint32_t>(tables.coop[i].states()) >= states &&
                    (smallest < 0 || tables.coop[i].states() < tables.coop[smallest].states()))
                    smallest = static_cast<int>(i);
            CHECK(ps.coop == (same_EJ ? smallest : -1));
            CHECK((ps.coop >= 0) == (ps.coop_max_n > 0));
            CHECK(ps.lat < 0 || ps.mid < 0 || ps.lat_max_n <= ps.mid_max_n);
            CHECK(states >= 80 || tables.variants[ps.main].G >= 16);
        }
    CHECK(msvplan::choose(tables, 4097, true, -1, cus, blocks_of).main == -1);
    CHECK(!asked_mid);
    std::printf("  plan policy: %zu recorded profiles and %zu variant_for points on %d CUs; 1..4096 states swept\n",
                rec["records"].array.size(), points, cus);
}

// 9b. the fused-grid decision, from the rules in msv_plan.cpp's comments
static void check_fused_grid(const msvplan::Tables& tables) {
    using msvplan::GridChoice;
    using msvplan::GridProfile;
    const int coop1400 = 2, lat1400 = variant_index("msv_g64_s24_w16_p6_d1");  // 1464 and 1536 states
    CHECK(tables.coop[coop1400].states() == 1464 && lat1400 >= 0);
    const GridProfile p{1400, false, true, 512};
    auto run = [&](std::vector<GridProfile> g, uint64_t n, bool host_residues = false, uint32_t most = 1) {
        return msvplan::fused_grid(tables, g.data(), static_cast<uint32_t>(g.size()), n, host_residues, most);
    };
    auto is = [](GridChoice c, int kind, int index) { return c.kind == kind && c.index == index; };
    const GridProfile small{100, false, true, 384}, forced{1400, true, true, 0}, other_EJ{1400, false, false, 0},
        no_coop{1400, false, true, 0};
    CHECK(is(run({p, small, p}, 3), GridChoice::kCoopFused, coop1400));  // the layout of the largest model
    CHECK(is(run({p}, 3), GridChoice::kPerProfile, -1));                 // a single profile
    // n x profiles at 2048 and 2049 (above every cooperative range)
    CHECK(is(run({p, p}, 1024), GridChoice::kLatencyFused, lat1400));
    CHECK(is(run({p, p, p}, 683), GridChoice::kPerProfile, -1));
    CHECK(is(run({p, forced, p}, 3), GridChoice::kPerProfile, -1));
    CHECK(is(run({p, other_EJ, p}, 3), GridChoice::kLatencyFused, lat1400));
    // workgroups of a launch at and one above the smallest coop_max_n
    CHECK(is(run({p, small, p}, 128), GridChoice::kCoopFused, coop1400));
    CHECK(is(run({p, small, p}, 129), GridChoice::kLatencyFused, lat1400));
    CHECK(is(run(std::vector<GridProfile>(40, small), 12), GridChoice::kCoopFused, 0));  // 32 profiles per launch
    CHECK(is(run(std::vector<GridProfile>(40, small), 13), GridChoice::kLatencyFused, variant_index("msv_g64_s4_w16_p1_d1")));
    CHECK(is(run({p, no_coop}, 3), GridChoice::kLatencyFused, lat1400));
    CHECK(is(run({p, p}, 3, true), GridChoice::kLatencyFused, lat1400));  // residues read in place
    // a handle listed 8 and 9 times: the latency layout holds a counter slot per entry, the cooperative none
    CHECK(is(run(std::vector<GridProfile>(9, no_coop), 3, false, 8), GridChoice::kLatencyFused, lat1400));
    CHECK(is(run(std::vector<GridProfile>(9, no_coop), 3, false, 9), GridChoice::kPerProfile, -1));
    CHECK(is(run(std::vector<GridProfile>(9, p), 3, false, 9), GridChoice::kCoopFused, coop1400));
    CHECK(is(run({GridProfile{4096, false, true, 0}, p}, 3), GridChoice::kLatencyFused, variant_index("msv_g64_s64_w12_p2_d1")));
}

// 9c. plan_pieces: the cuts of the function as it stood in msv_device.cpp (printed by a scratch build of it),
// and its properties on those and on random CSRs
struct PieceCase {
    const char* name;
    uint32_t first_den, growth;
    std::vector<uint64_t> offsets, cuts;
};

static std::vector<uint64_t> csr(uint64_t base, std::initializer_list<std::pair<uint64_t, uint64_t>> runs) {
    std::vector<uint64_t> o{base};  // runs of (count, length)
    for (const auto& r : runs)
        for (uint64_t i = 0; i < r.first; ++i) o.push_back(o.back() + r.second);
    return o;
}

static std::vector<uint64_t> checked_pieces(const std::vector<uint64_t>& offsets, uint32_t first_den, uint32_t growth) {
    const uint64_t n = offsets.size() - 1;
    const std::vector<uint64_t> cut = msvplan::plan_pieces(offsets.data(), n, offsets[n] - offsets[0], first_den, growth);
    bool ok = cut.size() >= 1 && cut.front() == 0 && cut.back() == n && (n == 0) == (cut.size() == 1);
    for (size_t k = 0; ok && k + 1 < cut.size(); ++k)
        ok = cut[k] < cut[k + 1] && cut[k + 1] <= n && offsets[cut[k + 1]] - offsets[cut[k]] < msvplan::kChunkBytes &&
             cut[k + 1] - cut[k] <= msvplan::kMaxLaunchSeqs - 1;
    CHECK(ok);
    return cut;
}

static void check_plan_pieces() {
    const PieceCase cases[] = {
        {"below 4 MiB", 4, 2, csr(0, {{1000, 1000}}), {0, 1000}},
        {"8 MiB, remainder joins", 4, 2, csr(0, {{8192, 1024}}), {0, 2048, 8192}},
        {"8 MiB, first_den 0", 0, 2, csr(0, {{8192, 1024}}), {0, 8192}},
        {"8 MiB, growth 1, remainder stays", 4, 1, csr(0, {{8192, 1024}}), {0, 2048, 4096, 6144, 8192}},
        {"9000 x 1024, growth 1", 4, 1, csr(0, {{9000, 1024}}), {0, 2250, 4500, 6750, 9000}},
        {"a sequence longer than the first piece", 4, 2, csr(0, {{1, 5u << 20}, {3000, 1024}}), {0, 1, 3001}},
        {"empty sequences around and inside", 4, 2,
         csr(0, {{2000, 0}, {3000, 1000}, {500, 0}, {3000, 1000}, {2000, 0}}), {0, 3500, 10500}},
        {"all empty", 4, 2, csr(0, {{5, 0}}), {0, 5}},
        {"offsets from 12345", 4, 2, csr(12345, {{40000, 1000}}), {0, 10000, 40000}},
        {"first_den 8", 8, 2, csr(0, {{40000, 1000}}), {0, 5000, 15000, 40000}},
        {"growth 3", 8, 3, csr(7, {{40000, 1000}}), {0, 5000, 20000, 40000}},
        {"one sequence of 6 MiB", 4, 2, csr(0, {{1, 6u << 20}}), {0, 1}},
        {"10 GB: the chunk limit", 4, 2, csr(0, {{100000, 102400}}), {0, 25000, 66932, 100000}},
    };
    for (const PieceCase& c : cases) {
        const bool same = checked_pieces(c.offsets, c.first_den, c.growth) == c.cuts;
        if (!same) std::printf("  plan_pieces: %s\n", c.name);
        CHECK(same);
    }
    CHECK(checked_pieces({0}, 4, 2) == std::vector<uint64_t>{0});  // no sequences
    std::mt19937_64 rng(23);
    for (int k = 0; k < 200; ++k) {
        const uint64_t n = 1 + rng() % 3000, scale = 1ull << (rng() % 23);  // up to ~12 GB
        std::vector<uint64_t> o{rng() % 1000};
        for (uint64_t i = 0; i < n; ++i) o.push_back(o.back() + (rng() % 4 ? rng() % (2 * scale) : 0));
        checked_pieces(o, static_cast<uint32_t>(rng() % 9), static_cast<uint32_t>(1 + rng() % 3));
    }
}

// 9d. rebase_offsets against a plain loop, bit for bit; the slots around the written range stay untouched
static void check_rebase(const char* name, const std::vector<uint64_t>& o, uint64_t first, uint64_t last) {
    const uint64_t kGuard = 0xfeedfacecafebeefull;
    std::vector<uint64_t> got(last - first + 3, kGuard), want(last - first + 3, kGuard);  // exact heap size: ASan
    msvplan::rebase_offsets(o.data(), first, last, got.data() + 1);
    for (uint64_t i = first; i <= last; ++i) want[1 + i - first] = o[i] - o[first];
    if (got != want) std::printf("  rebase_offsets: %s\n", name);
    CHECK(got == want);
}

static void check_rebase_offsets() {
    const uint64_t high = (1ull << 33) + 5;
    check_rebase("first offset 0", csr(0, {{50, 7}, {3, 0}, {20, 1000}}), 0, 73);
    check_rebase("first offset 2^33 + 5", csr(high, {{50, 7}, {3, 0}, {20, 1000}}), 0, 73);
    check_rebase("a sub-range", csr(high, {{50, 7}, {3, 0}, {20, 1000}}), 11, 60);
    check_rebase("empty sequences at both ends", csr(12, {{4, 0}, {30, 9}, {5, 0}}), 2, 37);
    check_rebase("empty sequences at both ends, whole", csr(12, {{4, 0}, {30, 9}, {5, 0}}), 0, 39);
    check_rebase("n = 1", csr(high, {{1, 300}}), 0, 1);
    check_rebase("n = 1 inside", csr(3, {{9, 300}}), 4, 5);
    check_rebase("n = 1, empty", csr(3, {{1, 0}}), 0, 1);
}

// 9e. plan_call: the mode the flags of msv_score_batch gave before the plan existed (zres / small / pipe,
// printed by a scratch build of them for these inputs), and the layout of the call's staging words
enum { kWantInPlace, kWantSmall, kWantCopiedOnePiece, kWantPipeline };

static void check_call_plan(const char* name, const std::vector<uint64_t>& o, bool in_place, uint32_t first_den,
                            uint32_t growth, int want) {
    using msvplan::CallPlan;
    const uint64_t n = o.size() - 1, total = o[n] - o[0];
    const CallPlan c = msvplan::plan_call(o.data(), n, total, in_place, first_den, growth);
    const size_t P = c.pieces();
    const CallPlan::Mode mode = want == kWantInPlace ? CallPlan::kInPlace : want == kWantSmall ? CallPlan::kSmall : CallPlan::kCopied;
    bool ok = c.mode == mode && c.pipeline == (want == kWantPipeline) && c.n == n;
    ok = ok && c.cut == checked_pieces(o, in_place ? 0 : first_den, growth);
    ok = ok && c.res_words == (want == kWantSmall ? (total + 7) / 8 : 0) && c.res_words * 8 >= (want == kWantSmall ? total : 0);
    // regions of the staging words, in order: every piece's offsets, the small call's residues, the error word
    std::vector<std::pair<uint64_t, uint64_t>> regions;  // [begin, end)
    std::vector<uint64_t> staged(c.staged_words(), 0);    // exact heap size: a write past the layout is ASan's
    for (size_t k = 0; k < P; ++k) {
        ok = ok && c.offsets_word(k) == c.cut[k] + k;
        regions.push_back({c.cut[k] + k, c.cut[k + 1] + k + 1});
        msvplan::rebase_offsets(o.data(), c.cut[k], c.cut[k + 1], staged.data() + c.offsets_word(k));
        ok = ok && staged[c.cut[k] + k] == 0 && staged[c.cut[k + 1] + k] == o[c.cut[k + 1]] - o[c.cut[k]];
    }
    regions.push_back({c.small_res_word(), c.small_res_word() + c.res_words});
    regions.push_back({c.err_word(), c.err_word() + 1});
    uint64_t at = 0;
    for (const auto& r : regions) {  // back to back from word 0: none overlaps another, none leaves a gap
        ok = ok && r.first == at && r.second >= r.first;
        at = r.second;
    }
    ok = ok && at == c.staged_words() && c.staged_words() == n + P + c.res_words + 1 &&
         c.upload_words() == n + P + c.res_words && c.err_word() >= c.upload_words();
    if (!ok) std::printf("  plan_call: %s (n = %llu, total = %llu)\n", name, static_cast<unsigned long long>(n),
                         static_cast<unsigned long long>(total));
    CHECK(ok);
}

// ~12,000 sequences of ~500 residues, 2,000 empty records and one 150,000-residue record placed on the cuts of
// the 4/2 plan (as tests/test_gpu_configs.py test_host_pipeline_piece_edges does)
static std::vector<uint64_t> pipeline_offsets() {
    std::mt19937_64 rng(41);
    std::vector<uint64_t> lens(12000);
    for (auto& L : lens) L = 300 + rng() % 401;
    std::vector<uint64_t> o{0};
    for (uint64_t L : lens) o.push_back(o.back() + L);
    const std::vector<uint64_t> cut = msvplan::plan_pieces(o.data(), lens.size(), o.back(), 4, 2);
    CHECK(cut.size() == 3);
    const size_t edge = cut.size() > 2 ? cut[1] : lens.size() / 4;
    lens.insert(lens.begin() + edge, 150000);  // the long record straddles the first cut
    lens.insert(lens.begin() + edge, 700, 0);  // empty records before it, after it, and at both ends
    lens.insert(lens.begin() + edge + 701, 700, 0);
    lens.insert(lens.begin(), 300, 0);
    lens.insert(lens.end(), 300, 0);
    std::vector<uint64_t> out{77};
    for (uint64_t L : lens) out.push_back(out.back() + L);
    return out;
}

static void check_call_plans() {
    using msvplan::kSmallCall;
    for (uint64_t n : {1, 3})
        for (uint64_t total : {uint64_t(0), uint64_t(1), uint64_t(7), uint64_t(8), uint64_t(9), kSmallCall, kSmallCall + 1}) {
            std::vector<uint64_t> o{5};  // total residues over n sequences, the remainder in the last
            for (uint64_t i = 0; i < n; ++i) o.push_back(o.back() + total / n + (i + 1 == n ? total % n : 0));
            check_call_plan("small", o, false, 4, 2, total <= kSmallCall ? kWantSmall : kWantCopiedOnePiece);
        }
    const std::vector<uint64_t> o = pipeline_offsets();
    CHECK(o.size() - 1 == 14001 && o.back() - o[0] >= msvplan::kPipelineMin);
    check_call_plan("pipeline 4/2", o, false, 4, 2, kWantPipeline);
    check_call_plan("pipeline 1/1", o, false, 1, 1, kWantCopiedOnePiece);
    check_call_plan("in place 4/2", o, true, 4, 2, kWantInPlace);
    check_call_plan("in place 1/1", o, true, 1, 1, kWantInPlace);
    CHECK(msvplan::plan_call(o.data(), o.size() - 1, o.back() - o[0], false, 4, 2).pieces() == 2);
    CHECK(msvplan::plan_call(o.data(), o.size() - 1, o.back() - o[0], true, 4, 2).pieces() == 1);
    // the in-place rule's two thresholds
    CHECK(msvplan::in_place_wins(300, 1ull << 30) && !msvplan::in_place_wins(299, 16ull << 20) &&
          msvplan::in_place_wins(299, (16ull << 20) - 1));
}

// 9f. the multi-device chunks are plan_pieces' with first_den = 0: a shard under 4 GiB is one piece (what
// msv_multi.cpp's own greedy loop gave), and 10 GiB in 1 MiB steps is cut into pieces under kChunkBytes that
// are as long as the limit allows (the greedy loop's cuts)
static void check_multi_chunks() {
    CHECK((checked_pieces(csr(9, {{4000, 1u << 20}}), 0, 1) == std::vector<uint64_t>{0, 4000}));  // 3.9 GiB
    CHECK((checked_pieces(pipeline_offsets(), 0, 1) == std::vector<uint64_t>{0, 14001}));
    const std::vector<uint64_t> o = csr(0, {{10240, 1u << 20}});
    const std::vector<uint64_t> cut = checked_pieces(o, 0, 1);
    std::vector<uint64_t> greedy{0};
    for (uint64_t a = 0; a < 10240;) {
        uint64_t b = a + 1;
        while (b < 10240 && o[b + 1] - o[a] < msvplan::kChunkBytes) ++b;
        greedy.push_back(a = b);
    }
    CHECK(cut == greedy && cut.size() == 4);
    for (size_t k = 0; k + 1 < cut.size(); ++k) CHECK(o[cut[k + 1]] - o[cut[k]] < msvplan::kChunkBytes);
}

static void check_plan_policy(const std::string& root) {
    const msvplan::Tables tables = plan_tables();
    CHECK(tables.variants.size() >= 80 && tables.coop.size() == 5);
    check_recorded_plans(root, tables);
    check_fused_grid(tables);
    check_plan_pieces();
    check_rebase_offsets();
    check_call_plans();
    check_multi_chunks();
    std::printf("  host staging: rebase_offsets on 8 ranges, plan_call on 18 calls, the multi-device chunks\n");
}

int main(int argc, char** argv) {
    const std::string root = argc > 1 ? argv[1] : ".";
    char tmpl[] = "/tmp/msv_sanitize_XXXXXX";
    const char* tmp = mkdtemp(tmpl);
    if (!tmp) return 2;
    const std::string dir = tmp;

    // 1. every profile parses; precompute + CPU DP equal the reference's golden scores bit for bit
    std::vector<std::string> profiles;
    if (DIR* d = opendir((root + "/data/profile_HMMs").c_str())) {
        while (dirent* e = readdir(d)) {
            const std::string n = e->d_name;
            if (n.size() > 4 && n.substr(n.size() - 4) == ".hmm") profiles.push_back(n);
        }
        closedir(d);
    }
    CHECK(profiles.size() == 24);
    check_scores(root, "fasta_like_example.fsa", "example_scores.tsv", profiles);
    check_scores(root, "random_FASTA.fsa", "random_fasta_scores.tsv", {"100.hmm", "1400.hmm", "2405.hmm"});
    {
        Table t;
        CHECK(load_table(root + "/data/profile_HMMs/100.hmm", t));
        CHECK(score(t, nullptr, 0) == -std::numeric_limits<float>::infinity());  // empty -> -inf
    }

    // 2. .hmm edge cases: missing, truncated anywhere, last line without its newline, garbage
    {
        msv_hmm* h = nullptr;
        CHECK(msv_hmm_read((root + "/data/profile_HMMs/none.hmm").c_str(), &h) == MSV_ERR_IO);
        const std::string text = slurp(root + "/data/profile_HMMs/100.hmm");
        Table ref;
        CHECK(load_table(root + "/data/profile_HMMs/100.hmm", ref));
        std::mt19937 rng(7);
        int ok_cuts = 0;
        for (int k = 0; k < 64; ++k) {
            const size_t cut = k < 8 ? static_cast<size_t>(k) : rng() % text.size();
            spit(dir + "/cut.hmm", text.substr(0, cut));
            h = nullptr;
            const msv_status s = msv_hmm_read((dir + "/cut.hmm").c_str(), &h);
            CHECK((s == MSV_OK) == (h != nullptr));
            if (h) {
                ++ok_cuts;
                msv_hmm_destroy(h);
            }
        }
        std::printf("  truncated 100.hmm: %d of 64 cuts parsed, the rest refused\n", ok_cuts);
        std::string no_nl = text;
        while (!no_nl.empty() && (no_nl.back() == '\n' || no_nl.back() == '\r')) no_nl.pop_back();
        spit(dir + "/nonl.hmm", no_nl);
        Table t;
        CHECK(load_table(dir + "/nonl.hmm", t));
        CHECK(t.M == ref.M && std::memcmp(t.e.data(), ref.e.data(), t.e.size() * 4) == 0);
        spit(dir + "/garbage.hmm", "HMMER3/f\nNAME x\nLENG abc\n");
        h = nullptr;
        CHECK(msv_hmm_read((dir + "/garbage.hmm").c_str(), &h) != MSV_OK && h == nullptr);
        std::remove((dir + "/cut.hmm").c_str());
        std::remove((dir + "/nonl.hmm").c_str());
        std::remove((dir + "/garbage.hmm").c_str());
    }

    // 3. FASTA: the golden edge cases, then first-line / EOF cases
    {
        Parsed p = parse_text(dir, "edge.fsa", slurp(root + "/tests/golden/edge_cases.fsa"));
        CHECK(p.status == MSV_OK);
        CHECK((p.lengths == std::vector<uint64_t>{20, 0, 5, 12, 10}));
        CHECK(p.rejected == 5);
        CHECK(static_cast<uint8_t>(p.codes[20 + 2]) == 255);  // '#' inside a record: rejected at scoring
        CHECK(parse_text(dir, "empty.fsa", "").status == MSV_OK);
        CHECK(parse_text(dir, "empty.fsa", "").lengths.empty());
        CHECK(parse_text(dir, "nohdr.fsa", "ACDE\n>x\nAC\n").status == MSV_ERR_PARSE);
        p = parse_text(dir, "blank.fsa", "\n\n>x\nAC");
        CHECK(p.status == MSV_OK && (p.lengths == std::vector<uint64_t>{2}));
        p = parse_text(dir, "hdronly.fsa", ">only header");
        CHECK(p.status == MSV_OK && (p.lengths == std::vector<uint64_t>{0}));
        p = parse_text(dir, "gt.fsa", ">a\nAC\n>");
        CHECK(p.status == MSV_OK && p.lengths.size() == 2 && p.lengths[0] == 2);
        msv_fasta* f = nullptr;
        CHECK(msv_fasta_read((dir + "/missing.fsa").c_str(), &f) == MSV_ERR_IO && f == nullptr);
    }

    // 4. a file large enough for the chunked multi-threaded reader (> 4 MiB per chunk), every record
    //    and every rejection known in advance
    {
        static const char kAA[] = "ACDEFGHIKLMNPQRSTVWY";
        std::mt19937_64 rng(11);
        std::string text, want;
        std::vector<uint64_t> lengths;
        size_t rejected = 0;
        while (text.size() < (40u << 20)) {
            const size_t L = rng() % 3000;
            const bool bad = rng() % 17 == 0;
            text += ">r" + std::to_string(lengths.size() + rejected) + "\n";
            std::string seq;
            for (size_t i = 0; i < L; ++i) seq += kAA[rng() % 20];
            if (bad) seq.insert(seq.size() / 2, 1, 'x');
            for (size_t i = 0; i < seq.size(); i += 60) text += seq.substr(i, 60) + "\n";
            if (bad) {
                ++rejected;
            } else {
                lengths.push_back(L);
                for (char c : seq) want += static_cast<char>(std::strchr(kAA, c) - kAA);
            }
        }
        Parsed p = parse_text(dir, "big.fsa", text);
        CHECK(p.status == MSV_OK);
        CHECK(p.lengths == lengths);
        CHECK(p.rejected == rejected);
        CHECK(p.codes == want);
        std::printf("  chunked reader: %zu MiB, %zu records, %zu rejected\n", text.size() >> 20, lengths.size(),
                    rejected);
    }

    // 5. shard bounds: cover, monotone, empty batches and more shards than sequences
    {
        std::vector<uint64_t> off{0, 5, 5, 5, 100, 101, 400};
        for (uint32_t shards : {1u, 2u, 3u, 6u, 8u, 64u}) {
            std::vector<uint64_t> b(shards + 1, 777);
            CHECK(msv_shard_bounds(off.data(), off.size() - 1, shards, b.data()) == MSV_OK);
            CHECK(b[0] == 0 && b[shards] == off.size() - 1);
            for (uint32_t k = 0; k < shards; ++k) CHECK(b[k] <= b[k + 1]);
        }
        std::vector<uint64_t> b(5, 777);
        CHECK(msv_shard_bounds(nullptr, 0, 4, b.data()) == MSV_OK);
        for (uint64_t x : b) CHECK(x == 0);
        CHECK(msv_shard_bounds(off.data(), 6, 0, b.data()) == MSV_ERR_INVALID_ARGUMENT);
    }

    // 7. the Viterbi stage's host side: table builder + CPU DP on every profile, both insert
    // modes, edge lengths; the MSV reduction (m->m = 1, every other transition impossible) equals the MSV DP
    {
        std::mt19937 rng(11);
        for (const std::string& prof : profiles) {
            msv_hmm* h = nullptr;
            CHECK(msv_hmm_read((root + "/data/profile_HMMs/" + prof).c_str(), &h) == MSV_OK);
            if (!h) continue;
            const size_t M = msv_hmm_model_length(h);
            std::vector<float> msc(20 * M), isc(20 * M), tsc(7 * M);
            float b = 0, c = 0, j = 0;
            for (int mode : {0, 1}) {
                CHECK(msv_hmm_viterbi_scores(h, mode, msc.data(), isc.data(), tsc.data(), &b, &c, &j) == MSV_OK);
                for (size_t L : {size_t(0), size_t(1), size_t(2), size_t(65), size_t(300)}) {
                    std::vector<uint8_t> codes(L);
                    for (auto& x : codes) x = static_cast<uint8_t>(rng() % 20);
                    float sc = 0;
                    CHECK(msv_vit_cpu_score(msc.data(), mode ? isc.data() : nullptr, tsc.data(), static_cast<uint32_t>(M),
                                            b, c, j, codes.data(), L, &sc) == MSV_OK);
                    CHECK(L > 0 ? std::isfinite(sc) : sc == -std::numeric_limits<float>::infinity());
                }
            }
            std::vector<float> red(7 * M, -std::numeric_limits<float>::infinity());
            for (size_t k = 0; k < M; ++k) red[k * 7] = 0.0f;
            std::vector<uint8_t> codes(200);
            for (auto& x : codes) x = static_cast<uint8_t>(rng() % 20);
            float v = 0;
            CHECK(msv_vit_cpu_score(msc.data(), nullptr, red.data(), static_cast<uint32_t>(M), b, c, j, codes.data(),
                                    codes.size(), &v) == MSV_OK);
            const float m = msv_host::run_on_sequence(msc.data(), M, b, c, j, codes.data(), codes.size());
            CHECK(std::memcmp(&v, &m, sizeof(float)) == 0);
            const uint8_t bad[3] = {1, 20, 2};
            CHECK(msv_vit_cpu_score(msc.data(), nullptr, tsc.data(), static_cast<uint32_t>(M), b, c, j, bad, 3, &v) ==
                  MSV_ERR_BAD_RESIDUE);
            msv_hmm_destroy(h);
        }
    }

    // 8. the kernel-layout table builders (table_layout.cpp) on compiled geometries, at R = capacity,
    // capacity - 1 and 1 real states
    check_layouts();

    // 9. the MSV plan policy (msv_plan.cpp): recorded plans, the fused-grid decision, the pipeline pieces
    check_plan_policy(root);

    rmdir(dir.c_str());
    if (failures) {
        std::printf("sanitize_host: %d check(s) failed\n", failures);
        return 1;
    }
    std::printf("sanitize_host passed\n");
    return 0;
}
