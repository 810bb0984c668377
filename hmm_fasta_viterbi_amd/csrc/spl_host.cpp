// spl_host.cpp -- the split stage on the host (msv.h states the model): the region test, the float64
// Forward twin with D, the definition of a sample on plain arrays, the clustering.  Host only, no HIP.  Built with
// -ffp-contract=off (spl_host.h says why).
#include "spl_host.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <numeric>

#include "host_cpu.h"

namespace msv_host {

namespace {

enum { MM, MI_, MD, IM, II_, DM, DD };

inline double odds(float score) { return std::exp(static_cast<double>(score)); }  // exp(-inf) = 0

constexpr double kBig = 0x1p256, kDown = 0x1p-256;
constexpr double kLn2 = 0.69314718055994530942;

}  // namespace

float spl_odds_of(float score) { return static_cast<float>(odds(score)); }

std::vector<float> spl_odds(const float* tsc, uint32_t model_length) {
    const size_t M = model_length, K = M - 1;
    std::vector<float> t(M * 7, 0.0f);
    for (size_t k = 1; k < K; ++k)
        for (int j = 0; j < 7; ++j) t[k * 7 + j] = spl_odds_of(tsc[k * 7 + j]);
    return t;
}

SplSample spl_sample_on_arrays(const float* fM, const float* fI, const float* fD, const uint32_t* records, size_t Le,
                               size_t M, const SplOdds& o, uint64_t key) {
    SplSample s;
    const float* plane[3] = {fM, fI, fD};
    const bool whole = spl_sample(
        Le, static_cast<uint32_t>(M - 1),
        [&](int p, uint64_t i, uint32_t k) -> float { return plane[p][(i - 1) * M + k]; },
        [&](uint64_t i, int w) -> uint32_t { return records[i * 6 + static_cast<size_t>(w)]; }, o, key,
        [&](char c, uint64_t, uint32_t) { s.ops.push_back(static_cast<uint8_t>(c)); },
        [&](uint32_t i_from, uint32_t i_to, uint32_t k_from, uint32_t k_to, uint32_t len) {
            s.segments.push_back(msv_spl_segment{i_from, i_to, k_from, k_to});
            msv_vit_domain d{};
            d.i_from = i_from, d.i_to = i_to, d.k_from = k_from, d.k_to = k_to, d.ops_len = len;
            s.domains.push_back(d);
        });
    s.truncated = !whole;
    // a truncated sample keeps the domains it finished; the ops of the one under way are dropped
    uint64_t kept = 0;
    for (const msv_vit_domain& d : s.domains) kept += d.ops_len;
    s.ops.resize(kept);
    std::reverse(s.ops.begin(), s.ops.end());
    std::reverse(s.segments.begin(), s.segments.end());
    std::reverse(s.domains.begin(), s.domains.end());
    uint64_t at = 0;
    for (msv_vit_domain& d : s.domains) {
        d.ops_begin = at;
        at += d.ops_len;
    }
    return s;
}

void spl_forward_on_envelope(const FwdModel& m, const uint8_t* codes, size_t L, size_t Lc, double* score, double* fM,
                             double* fI, double* fD, double* specials, int32_t* exponents) {
    if (L == 0) {
        if (score) *score = -std::numeric_limits<double>::infinity();
        if (specials) specials[0] = 1.0, specials[1] = specials[2] = specials[4] = 0.0, specials[3] = 0.0;
        if (exponents) exponents[0] = 0;
        return;
    }
    const size_t M = m.M, K = M - 1;
    float lf, mf;
    msv_sequence_transitions(Lc, &lf, &mf);
    const double loop = odds(lf), move = odds(mf);
    const double* xt = m.xt.data();
    std::vector<double> Mp(M, 0.0), Ip(M, 0.0), Dp(M, 0.0), Mc(M, 0.0), Ic(M, 0.0), Dc(M, 0.0);
    double N = 1.0, J = 0.0, C = 0.0, B = N * move;
    int32_t e2 = 0;
    auto put = [&](size_t i, double E) {
        if (specials) {
            double* s = specials + i * 5;
            s[0] = N, s[1] = J, s[2] = C, s[3] = B, s[4] = E;
        }
        if (exponents) exponents[i] = e2;
    };
    put(0, 0.0);
    for (size_t i = 0; i < L; ++i) {
        const double* xm = m.xm.data() + static_cast<size_t>(codes[i]) * M;
        const double* xi = m.xi.data() + static_cast<size_t>(codes[i]) * M;
        const double Bt = B * m.tBM;
        double E = 0.0;
        Mc[0] = Ic[0] = Dc[0] = 0.0;
        for (size_t k = 1; k <= K; ++k) {
            const double* tin = xt + (k - 1) * 7;
            const double* tout = xt + k * 7;
            Mc[k] = xm[k] * (Mp[k - 1] * tin[MM] + Ip[k - 1] * tin[IM] + Dp[k - 1] * tin[DM] + Bt);
            Ic[k] = xi[k] * (Mp[k] * tout[MI_] + Ip[k] * tout[II_]);
            Dc[k] = Mc[k - 1] * tin[MD] + Dc[k - 1] * tin[DD];
            E += Mc[k] + Dc[k];
        }
        N *= loop;
        J = J * loop + E * m.tEJ;
        C = C * loop + E * m.tEC;
        B = (N + J) * move;
        if (E > kBig) {
            for (size_t k = 1; k <= K; ++k) Mc[k] *= kDown, Ic[k] *= kDown, Dc[k] *= kDown;
            N *= kDown, J *= kDown, C *= kDown, B *= kDown, E *= kDown;
            e2 += 256;
        }
        put(i + 1, E);
        if (fM) std::copy(Mc.begin(), Mc.end(), fM + i * M);
        if (fI) std::copy(Ic.begin(), Ic.end(), fI + i * M);
        if (fD) std::copy(Dc.begin(), Dc.end(), fD + i * M);
        Mp.swap(Mc), Ip.swap(Ic), Dp.swap(Dc);
    }
    if (score) *score = std::log(C * move) + static_cast<double>(e2) * kLn2;
}

bool dom_is_multidomain(const float* begin, const float* end, uint32_t i_from, uint32_t i_to, float rt3) {
    // Bsum(z) downward from i_to, kept; then Esum(z) upward
    const size_t n = static_cast<size_t>(i_to) - i_from + 1;
    std::vector<float> bsum(n);
    float b = 0.0f;
    for (size_t j = n; j-- > 0;) {
        b = b + begin[i_from - 1 + j];
        bsum[j] = b;
    }
    float e = 0.0f, best = 0.0f;
    for (size_t j = 0; j < n; ++j) {
        e = e + end[i_from - 1 + j];
        const float lo = e < bsum[j] ? e : bsum[j];
        if (lo > best) best = lo;
    }
    return best >= rt3;
}

std::vector<msv_spl_envelope> spl_cluster(const msv_spl_segment* seg, size_t n, uint32_t n_samples,
                                          const SplClusterRule& r) {
    auto overlap_ok = [&](uint32_t a1, uint32_t a2, uint32_t b1, uint32_t b2) {
        const uint64_t lo = std::max(a1, b1), hi = std::min(a2, b2);
        const uint64_t ov = hi >= lo ? hi - lo + 1 : 0;
        const uint64_t la = static_cast<uint64_t>(a2) - a1 + 1, lb = static_cast<uint64_t>(b2) - b1 + 1;
        return static_cast<uint64_t>(r.ov_den) * ov >= static_cast<uint64_t>(r.ov_num) * std::min(la, lb);
    };
    auto diag_ok = [&](uint32_t ia, uint32_t ka, uint32_t ib, uint32_t kb) {
        const int64_t d = (static_cast<int64_t>(ia) - ka) - (static_cast<int64_t>(ib) - kb);
        return static_cast<uint64_t>(d < 0 ? -d : d) <= r.max_diagdiff;
    };
    auto linked = [&](const msv_spl_segment& a, const msv_spl_segment& b) {
        return overlap_ok(a.i_from, a.i_to, b.i_from, b.i_to) && overlap_ok(a.k_from, a.k_to, b.k_from, b.k_to) &&
               diag_ok(a.i_from, a.k_from, b.i_from, b.k_from) && diag_ok(a.i_to, a.k_to, b.i_to, b.k_to);
    };
    // connected components; a component's root is its lowest segment index
    std::vector<size_t> root(n);
    std::iota(root.begin(), root.end(), size_t{0});
    auto find = [&](size_t x) {
        while (root[x] != x) x = root[x] = root[root[x]];
        return x;
    };
    for (size_t a = 0; a < n; ++a)
        for (size_t b = a + 1; b < n; ++b) {
            const size_t ra = find(a), rb = find(b);
            if (ra != rb && linked(seg[a], seg[b])) root[std::max(ra, rb)] = std::min(ra, rb);
        }
    std::vector<msv_spl_envelope> out;
    std::vector<uint32_t> vals;
    for (size_t c = 0; c < n; ++c) {
        if (find(c) != c) continue;
        std::vector<size_t> mem;
        for (size_t a = c; a < n; ++a)
            if (find(a) == c) mem.push_back(a);
        const uint64_t count = mem.size();
        if (static_cast<uint64_t>(r.post_den) * count < static_cast<uint64_t>(r.post_num) * n_samples) continue;
        // the smallest (largest) value of a field whose frequency in the cluster reaches min_endpointp
        auto endpoint = [&](uint32_t msv_spl_segment::*f, bool smallest) {
            vals.clear();
            for (size_t a : mem) vals.push_back(seg[a].*f);
            std::sort(vals.begin(), vals.end());
            uint32_t best = smallest ? vals.front() : vals.back();
            bool found = false;
            for (size_t x = 0; x < vals.size();) {
                size_t y = x;
                while (y < vals.size() && vals[y] == vals[x]) ++y;
                if (static_cast<uint64_t>(r.end_den) * (y - x) >= static_cast<uint64_t>(r.end_num) * count &&
                    (!found || !smallest)) {
                    best = vals[x];
                    found = true;
                }
                x = y;
            }
            return best;
        };
        msv_spl_envelope e{};
        e.i_from = endpoint(&msv_spl_segment::i_from, true);
        e.i_to = endpoint(&msv_spl_segment::i_to, false);
        e.k_from = endpoint(&msv_spl_segment::k_from, true);
        e.k_to = endpoint(&msv_spl_segment::k_to, false);
        e.count = static_cast<uint32_t>(count);
        e.prob = static_cast<float>(count) / static_cast<float>(n_samples);
        out.push_back(e);
    }
    std::stable_sort(out.begin(), out.end(),
                     [](const msv_spl_envelope& a, const msv_spl_envelope& b) { return a.i_from < b.i_from; });
    return out;
}

}  // namespace msv_host

extern "C" {

msv_status msv_dom_is_multidomain(const float* begin, const float* end, uint64_t L, uint32_t i_from, uint32_t i_to,
                                  float rt3, int* multidomain) {
    if (!begin || !end || !multidomain || i_from < 1 || i_from > i_to || i_to > L) return MSV_ERR_INVALID_ARGUMENT;
    *multidomain = msv_host::dom_is_multidomain(begin, end, i_from, i_to, rt3) ? 1 : 0;
    return MSV_OK;
}

msv_status msv_spl_cpu_forward(const float* match_scores, const float* insert_scores, const float* transition_scores,
                               uint32_t model_length, float tr_B_Mk, float tr_E_C, float tr_E_J, const uint8_t* codes,
                               uint64_t Le, uint64_t Lc, double* score, double* fM, double* fI, double* fD,
                               double* specials, int32_t* exponents) {
    if (!match_scores || !transition_scores || model_length < 2 || (Le && !codes) || Lc < Le || Lc >= (1ull << 31))
        return MSV_ERR_INVALID_ARGUMENT;
    for (uint64_t i = 0; i < Le; ++i)
        if (codes[i] >= 20) return MSV_ERR_BAD_RESIDUE;
    const msv_host::FwdModel m = msv_host::fwd_model(match_scores, insert_scores, transition_scores, model_length,
                                                     tr_B_Mk, tr_E_C, tr_E_J);
    msv_host::spl_forward_on_envelope(m, codes, Le, Lc, score, fM, fI, fD, specials, exponents);
    return MSV_OK;
}

msv_status msv_spl_sample(const float* fM, const float* fI, const float* fD, const uint32_t* records,
                          const float* transition_scores, uint32_t model_length, float tr_B_Mk, float tr_E_C,
                          float tr_E_J, uint64_t Lc, uint64_t seed, uint32_t seq, uint32_t i_from, uint32_t i_to,
                          uint32_t sample, uint32_t* n_segments, uint64_t* n_ops, int* truncated,
                          msv_spl_segment* segments, msv_vit_domain* domains, uint8_t* ops) {
    if (!fM || !fI || !fD || !records || !transition_scores || model_length < 2 || !n_segments || !n_ops ||
        i_from < 1 || i_from > i_to || Lc < i_to || Lc >= (1ull << 31) || (ops != nullptr) != (domains != nullptr) ||
        (ops && !segments))
        return MSV_ERR_INVALID_ARGUMENT;
    const uint64_t Le = static_cast<uint64_t>(i_to) - i_from + 1;
    const std::vector<float> tr = msv_host::spl_odds(transition_scores, model_length);
    float loop, move;
    msv_sequence_transitions(Lc, &loop, &move);
    const msv_host::SplOdds o{tr.data(), msv_host::spl_odds_of(tr_B_Mk), msv_host::spl_odds_of(tr_E_C),
                              msv_host::spl_odds_of(tr_E_J), msv_host::spl_odds_of(loop)};
    msv_host::SplSample s = msv_host::spl_sample_on_arrays(fM, fI, fD, records, Le, model_length, o,
                                                           msv_host::spl_key(seed, seq, i_from, i_to, sample));
    if (truncated) *truncated = s.truncated ? 1 : 0;
    if (segments) {
        if (*n_segments < s.segments.size() || (ops && *n_ops < s.ops.size())) return MSV_ERR_INVALID_ARGUMENT;
        for (size_t j = 0; j < s.segments.size(); ++j) {
            msv_spl_segment g = s.segments[j];
            g.i_from += i_from - 1;
            g.i_to += i_from - 1;
            segments[j] = g;
        }
        if (ops) {
            std::copy(s.domains.begin(), s.domains.end(), domains);
            std::copy(s.ops.begin(), s.ops.end(), ops);
        }
    }
    *n_segments = static_cast<uint32_t>(s.segments.size());
    *n_ops = s.ops.size();
    return MSV_OK;
}

msv_status msv_spl_cluster(const msv_spl_segment* segments, uint64_t n_segments, uint32_t n_samples,
                           const msv_spl_cluster_options* options, uint32_t* n_envelopes,
                           msv_spl_envelope* envelopes) {
    if ((n_segments && !segments) || !n_envelopes || n_samples == 0) return MSV_ERR_INVALID_ARGUMENT;
    msv_spl_cluster_options o;
    if (!msv_host::read_sized(options, &o, sizeof(uint64_t))) return MSV_ERR_INVALID_ARGUMENT;
    msv_host::SplClusterRule r;
    if (o.min_overlap_den) r.ov_num = o.min_overlap_num, r.ov_den = o.min_overlap_den;
    if (o.max_diagdiff) r.max_diagdiff = o.max_diagdiff;
    if (o.min_posterior_den) r.post_num = o.min_posterior_num, r.post_den = o.min_posterior_den;
    if (o.min_endpointp_den) r.end_num = o.min_endpointp_num, r.end_den = o.min_endpointp_den;
    for (uint64_t j = 0; j < n_segments; ++j)
        if (segments[j].i_from > segments[j].i_to || segments[j].k_from > segments[j].k_to)
            return MSV_ERR_INVALID_ARGUMENT;
    const std::vector<msv_spl_envelope> env = msv_host::spl_cluster(segments, n_segments, n_samples, r);
    if (envelopes) {
        if (*n_envelopes < env.size()) return MSV_ERR_INVALID_ARGUMENT;
        std::copy(env.begin(), env.end(), envelopes);
    }
    *n_envelopes = static_cast<uint32_t>(env.size());
    return MSV_OK;
}

uint64_t msv_spl_item_bytes(uint32_t states_per_lane, uint64_t Le) {
    return msv_host::spl_item_bytes(states_per_lane, Le);
}

}  // extern "C"
