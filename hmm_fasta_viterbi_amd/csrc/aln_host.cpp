// aln_host.cpp -- the alignment stage on the host (msv.h states the model): the float64 posterior
// decoding of an envelope, the definition of the optimal-accuracy alignment, the fill kernel's gate bytes.  Host
// only, no HIP.
#include "aln_host.h"

#include <algorithm>
#include <cmath>
#include <limits>

#include "vit_trace_plan.h"

namespace msv_host {

namespace {

enum { MM, MI_, MD, IM, II_, DM, DD };  // file order m->m m->i m->d i->m i->i d->m d->d

inline double odds(float score) { return std::exp(static_cast<double>(score)); }  // exp(-inf) = 0

constexpr double kBig = 0x1p256, kDown = 0x1p-256;
constexpr double kLn2 = 0.69314718055994530942;

}  // namespace

void aln_decode_on_envelope(const FwdModel& m, const uint8_t* codes, size_t L, size_t Lc, double* score, double* ppM,
                            double* ppI, double* ppN, double* ppJ, double* ppC) {
    if (L == 0) {
        if (score) *score = -std::numeric_limits<double>::infinity();
        return;
    }
    const size_t M = m.M, K = M - 1;
    float lf, mf;
    msv_sequence_transitions(Lc, &lf, &mf);
    const double loop = odds(lf), move = odds(mf);
    const double* xt = m.xt.data();

    // Forward as decode_run_on_sequence, keeping every row: fM, fI of row i at [i][k], in the scale of fe[i]
    std::vector<double> fM((L + 1) * M, 0.0), fI((L + 1) * M, 0.0);
    std::vector<double> fN(L + 1), fJ(L + 1), fC(L + 1);
    std::vector<int64_t> fe(L + 1);
    {
        std::vector<double> Dp(M, 0.0), Dc(M, 0.0);
        double N = 1.0, J = 0.0, C = 0.0, B = N * move;
        int64_t e2 = 0;
        fN[0] = N, fJ[0] = J, fC[0] = C, fe[0] = 0;
        for (size_t i = 0; i < L; ++i) {
            const double* xm = m.xm.data() + static_cast<size_t>(codes[i]) * M;
            const double* xi = m.xi.data() + static_cast<size_t>(codes[i]) * M;
            const double* Mp = fM.data() + i * M;
            const double* Ip = fI.data() + i * M;
            double* Mc = fM.data() + (i + 1) * M;
            double* Ic = fI.data() + (i + 1) * M;
            const double Bt = B * m.tBM;
            double E = 0.0;
            Dc[0] = 0.0;
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
            Dp.swap(Dc);
            if (E > kBig) {
                for (size_t k = 1; k <= K; ++k) Mc[k] *= kDown, Ic[k] *= kDown, Dp[k] *= kDown;
                N *= kDown, J *= kDown, C *= kDown, B *= kDown;
                e2 += 256;
            }
            fN[i + 1] = N, fJ[i + 1] = J, fC[i + 1] = C, fe[i + 1] = e2;
        }
    }
    const double Zs = fC[L] * move;  // Z = Zs 2^fe[L]
    if (score) *score = std::log(Zs) + static_cast<double>(fe[L]) * kLn2;

    // Backward as decode_run_on_sequence; a row's bM, bI are combined with its fM, fI as soon as they stand
    std::vector<double> Mn(M + 1, 0.0), In(M + 1, 0.0), Mc(M + 1, 0.0), Ic(M + 1, 0.0), Dc(M + 2, 0.0);
    std::vector<double> P(M + 1, 0.0), H(M + 1, 0.0);
    double bJ = 0.0, bC = 0.0, bN = 0.0;
    int64_t be = 0;
    for (size_t i = L + 1; i-- > 0;) {
        double bB = 0.0;
        double lJ = 0.0, lC = 0.0, lN = 0.0;
        if (i == L) {
            std::fill(P.begin(), P.end(), 0.0);
            std::fill(H.begin(), H.end(), 0.0);
            bC = move;
            bJ = bN = 0.0;
        } else {
            const double* xm = m.xm.data() + static_cast<size_t>(codes[i]) * M;
            const double* xi = m.xi.data() + static_cast<size_t>(codes[i]) * M;
            double sigma = 0.0;
            for (size_t k = 1; k <= K; ++k) {
                P[k] = xm[k] * Mn[k];
                H[k] = k < K ? xi[k] * In[k] : 0.0;
                sigma += P[k];
            }
            if (sigma > kBig) {
                for (size_t k = 1; k <= K; ++k) P[k] *= kDown, H[k] *= kDown;
                bJ *= kDown, bC *= kDown, bN *= kDown, sigma *= kDown;
                be += 256;
            }
            bB = m.tBM * sigma;
            lJ = loop * bJ, lC = loop * bC, lN = loop * bN;
            bJ = lJ + move * bB;
            bC = lC;
            bN = lN + move * bB;
        }
        const double bE = m.tEJ * bJ + m.tEC * bC;
        Dc[K + 1] = 0.0;
        for (size_t k = K; k >= 1; --k) {
            const double* t = xt + k * 7;
            const double g = k < K ? P[k + 1] : 0.0, h = H[k];
            Dc[k] = (k >= 2 ? bE : 0.0) + t[DM] * g + t[DD] * Dc[k + 1];
            Mc[k] = bE + t[MM] * g + t[MI_] * h + t[MD] * Dc[k + 1];
            Ic[k] = t[IM] * g + t[II_] * h;
        }
        Mn.swap(Mc);
        In.swap(Ic);
        const int sh = static_cast<int>(fe[i] + be - fe[L]);
        if (i >= 1) {
            const double* fm = fM.data() + i * M;
            const double* fi = fI.data() + i * M;
            for (size_t k = 1; k <= K; ++k) {
                if (ppM) ppM[(i - 1) * M + k] = std::ldexp(fm[k] * Mn[k] / Zs, sh);
                if (ppI) ppI[(i - 1) * M + k] = k < K ? std::ldexp(fi[k] * In[k] / Zs, sh) : 0.0;
            }
            if (ppM) ppM[(i - 1) * M] = 0.0;
            if (ppI) ppI[(i - 1) * M] = 0.0;
        }
        if (i < L) {  // residue i + 1 emitted by N, J or C: the three terms of 1 - occ
            if (ppN) ppN[i] = std::ldexp(fN[i] * lN / Zs, sh);
            if (ppJ) ppJ[i] = std::ldexp(fJ[i] * lJ / Zs, sh);
            if (ppC) ppC[i] = std::ldexp(fC[i] * lC / Zs, sh);
        }
    }
}

AlnTrace aln_oa_on_envelope(const float* ppM, const float* ppI, const float* ppN, const float* ppJ, const float* ppC,
                            const float* tsc, size_t M, float tr_B_Mk, float tr_E_C, float tr_E_J, size_t Le,
                            size_t Lc) {
    // One max over the open candidates and one float add per cell; a source is the first candidate, in msv.h's
    // tie-break order, that EQUALS the max.  max is exact, so aln_kernel.hip finds the same bits on the same arrays.
    using namespace vittrace;
    constexpr float ninf = -std::numeric_limits<float>::infinity();
    auto via = [](float x, float t) { return std::isfinite(t) ? x : ninf; };
    const size_t K = M - 1;
    float loop, move;
    msv_sequence_transitions(Lc, &loop, &move);
    (void)loop;
    std::vector<float> Mv(M, ninf), Iv(M, ninf), Dv(M, ninf);
    std::vector<uint8_t> cell(Le * K);  // [row i-1][node k-1]
    std::vector<uint32_t> rec(Le);
    float J = ninf, C = ninf, N = 0.0f, B = via(0.0f, move);
    for (size_t i = 0; i < Le; ++i) {
        const float* pm = ppM + i * M;
        const float* pi = ppI + i * M;
        uint8_t* bits = cell.data() + i * K;
        const float Bt = via(B, tr_B_Mk);
        float E = ninf;
        for (size_t k = K; k >= 1; --k) {
            const float* tp = tsc + (k - 1) * 7;  // into node k from node k-1
            uint32_t b = 0;
            if (k < K) {
                const float* tk = tsc + k * 7;
                const float mi = via(Mv[k], tk[MI_]), ii = via(Iv[k], tk[II_]);
                const float iv = std::max(mi, ii);
                if (!(iv == mi)) b |= kIFromI;
                Iv[k] = iv + pi[k];
            } else {
                Iv[k] = ninf;  // no insert state at node LENG
            }
            const float cm = k > 1 ? via(Mv[k - 1], tp[MM]) : ninf, ci = k > 1 ? via(Iv[k - 1], tp[IM]) : ninf,
                        cd = k > 1 ? via(Dv[k - 1], tp[DM]) : ninf;
            const float mx = std::max(std::max(cm, ci), std::max(cd, Bt));
            b |= mx == cm ? kFromM : mx == ci ? kFromI : mx == cd ? kFromD : kFromB;
            Mv[k] = mx + pm[k];
            E = std::max(E, Mv[k]);
            bits[k - 1] = static_cast<uint8_t>(b);
        }
        Dv[1] = ninf;  // entered from node 0, which only B leaves
        for (size_t k = 2; k <= K; ++k) {
            const float* tp = tsc + (k - 1) * 7;
            const float md = via(Mv[k - 1], tp[MD]), dd = via(Dv[k - 1], tp[DD]);
            Dv[k] = std::max(md, dd);
            if (!(Dv[k] == md)) bits[k - 1] |= kDFromD;
        }
        size_t kE = 1;
        while (kE < K && !(Mv[kE] == E)) ++kE;  // the smallest k with M(i,k) == E(i)
        const float Jl = J + ppJ[i], Cl = C + ppC[i];
        J = std::max(Jl, via(E, tr_E_J));
        C = std::max(Cl, via(E, tr_E_C));
        N = N + ppN[i];
        const float Bn = via(N, move);
        B = std::max(Bn, via(J, move));
        rec[i] = static_cast<uint32_t>(kE) | (C == Cl ? 0u : kRecCFromE) | (J == Jl ? 0u : kRecJFromE) |
                 (B == Bn ? 0u : kRecBFromJ);
    }
    AlnTrace t;
    t.score = C;
    if (Le == 0 || !std::isfinite(t.score)) return t;
    aln_walk(
        Le, static_cast<uint32_t>(K), [&](uint64_t i, uint32_t k) -> uint32_t { return cell[(i - 1) * K + (k - 1)]; },
        [&](uint64_t i) -> uint32_t { return rec[i - 1]; },
        [&](char c, uint64_t i, uint32_t k) {
            t.ops.push_back(static_cast<uint8_t>(c));
            t.op_pp.push_back(c == 'M' ? ppM[(i - 1) * M + k] : c == 'I' ? ppI[(i - 1) * M + k] : 0.0f);
        },
        [&](uint32_t i_from, uint32_t i_to, uint32_t k_from, uint32_t k_to, uint32_t len) {
            msv_vit_domain d{};
            d.i_from = i_from, d.i_to = i_to, d.k_from = k_from, d.k_to = k_to, d.ops_len = len;
            t.domains.push_back(d);
        });
    std::reverse(t.ops.begin(), t.ops.end());
    std::reverse(t.op_pp.begin(), t.op_pp.end());
    std::reverse(t.domains.begin(), t.domains.end());
    uint64_t at = 0;
    for (msv_vit_domain& d : t.domains) {
        d.ops_begin = at;
        at += d.ops_len;
    }
    return t;
}

std::vector<uint32_t> aln_gates(const float* tsc, uint32_t model_length, float tr_B_Mk, int S) {
    const uint32_t K = model_length - 1;
    const size_t words = (static_cast<size_t>(S) + 3) / 4;
    std::vector<uint32_t> g(words * 64, 0u);
    for (uint32_t l = 0; l < 64; ++l)
        for (int q = 0; q < S; ++q) {
            const uint32_t k = l * static_cast<uint32_t>(S) + static_cast<uint32_t>(q) + 1;
            if (k > K) continue;
            uint32_t b = std::isfinite(tr_B_Mk) ? kGateBM : 0u;
            if (k > 1) {
                const float* tp = tsc + static_cast<size_t>(k - 1) * 7;
                b |= (std::isfinite(tp[MM]) ? kGateMM : 0u) | (std::isfinite(tp[IM]) ? kGateIM : 0u) |
                     (std::isfinite(tp[DM]) ? kGateDM : 0u) | (std::isfinite(tp[MD]) ? kGateMD : 0u) |
                     (std::isfinite(tp[DD]) ? kGateDD : 0u);
            }
            if (k < K) {
                const float* tk = tsc + static_cast<size_t>(k) * 7;
                b |= (std::isfinite(tk[MI_]) ? kGateMI : 0u) | (std::isfinite(tk[II_]) ? kGateII : 0u);
            }
            g[static_cast<size_t>(q / 4) * 64 + l] |= b << ((q % 4) * 8);
        }
    return g;
}

}  // namespace msv_host

extern "C" {

namespace {
msv_status check_envelope(const float* match_scores, const float* transition_scores, uint32_t model_length,
                          const uint8_t* codes, uint64_t Le, uint64_t Lc) {
    if (!match_scores || !transition_scores || model_length < 2 || (Le && !codes) || Lc < Le || Lc >= (1ull << 31))
        return MSV_ERR_INVALID_ARGUMENT;
    for (uint64_t i = 0; i < Le; ++i)
        if (codes[i] >= 20) return MSV_ERR_BAD_RESIDUE;
    return MSV_OK;
}

// The second call of the sizing protocol finds the first call's counts in the caller's variables.
msv_status give_trace(const msv_host::AlnTrace& t, float* oa_score, uint32_t* n_domains, uint64_t* n_ops,
                      msv_vit_domain* domains, uint8_t* ops, float* op_pp) {
    if (oa_score) *oa_score = t.score;
    if (domains) {
        if (*n_domains < t.domains.size() || *n_ops < t.ops.size()) return MSV_ERR_INVALID_ARGUMENT;
        std::copy(t.domains.begin(), t.domains.end(), domains);
        std::copy(t.ops.begin(), t.ops.end(), ops);
        std::copy(t.op_pp.begin(), t.op_pp.end(), op_pp);
    }
    *n_domains = static_cast<uint32_t>(t.domains.size());
    *n_ops = t.ops.size();
    return MSV_OK;
}
}  // namespace

msv_status msv_aln_cpu_decode(const float* match_scores, const float* insert_scores, const float* transition_scores,
                              uint32_t model_length, float tr_B_Mk, float tr_E_C, float tr_E_J, const uint8_t* codes,
                              uint64_t Le, uint64_t Lc, double* score, double* ppM, double* ppI, double* ppN,
                              double* ppJ, double* ppC) {
    const msv_status s = check_envelope(match_scores, transition_scores, model_length, codes, Le, Lc);
    if (s != MSV_OK) return s;
    const msv_host::FwdModel m = msv_host::fwd_model(match_scores, insert_scores, transition_scores, model_length,
                                                     tr_B_Mk, tr_E_C, tr_E_J);
    msv_host::aln_decode_on_envelope(m, codes, Le, Lc, score, ppM, ppI, ppN, ppJ, ppC);
    return MSV_OK;
}

msv_status msv_aln_oa(const float* ppM, const float* ppI, const float* ppN, const float* ppJ, const float* ppC,
                      const float* transition_scores, uint32_t model_length, float tr_B_Mk, float tr_E_C,
                      float tr_E_J, uint64_t Le, uint64_t Lc, float* oa_score, uint32_t* n_domains, uint64_t* n_ops,
                      msv_vit_domain* domains, uint8_t* ops, float* op_pp) {
    if (!transition_scores || model_length < 2 || !n_domains || !n_ops || Lc < Le || Lc >= (1ull << 31) ||
        (Le && (!ppM || !ppI || !ppN || !ppJ || !ppC)) || (domains == nullptr) != (ops == nullptr) ||
        (domains == nullptr) != (op_pp == nullptr))
        return MSV_ERR_INVALID_ARGUMENT;
    const msv_host::AlnTrace t = msv_host::aln_oa_on_envelope(ppM, ppI, ppN, ppJ, ppC, transition_scores, model_length,
                                                              tr_B_Mk, tr_E_C, tr_E_J, Le, Lc);
    return give_trace(t, oa_score, n_domains, n_ops, domains, ops, op_pp);
}

msv_status msv_aln_cpu_align(const float* match_scores, const float* insert_scores, const float* transition_scores,
                             uint32_t model_length, float tr_B_Mk, float tr_E_C, float tr_E_J, const uint8_t* codes,
                             uint64_t Le, uint64_t Lc, double* score, float* oa_score, uint32_t* n_domains,
                             uint64_t* n_ops, msv_vit_domain* domains, uint8_t* ops, float* op_pp) {
    if (!n_domains || !n_ops || (domains == nullptr) != (ops == nullptr) || (domains == nullptr) != (op_pp == nullptr))
        return MSV_ERR_INVALID_ARGUMENT;
    const msv_status s = check_envelope(match_scores, transition_scores, model_length, codes, Le, Lc);
    if (s != MSV_OK) return s;
    const size_t M = model_length;
    const msv_host::FwdModel m = msv_host::fwd_model(match_scores, insert_scores, transition_scores, model_length,
                                                     tr_B_Mk, tr_E_C, tr_E_J);
    std::vector<double> dM(Le * M, 0.0), dI(Le * M, 0.0), dN(Le, 0.0), dJ(Le, 0.0), dC(Le, 0.0);
    msv_host::aln_decode_on_envelope(m, codes, Le, Lc, score, dM.data(), dI.data(), dN.data(), dJ.data(), dC.data());
    // the float64 posteriors rounded to float32 once, then the definition
    std::vector<float> fM(dM.begin(), dM.end()), fI(dI.begin(), dI.end()), fN(dN.begin(), dN.end()),
        fJ(dJ.begin(), dJ.end()), fC(dC.begin(), dC.end());
    const msv_host::AlnTrace t = msv_host::aln_oa_on_envelope(fM.data(), fI.data(), fN.data(), fJ.data(), fC.data(),
                                                              transition_scores, M, tr_B_Mk, tr_E_C, tr_E_J, Le, Lc);
    return give_trace(t, oa_score, n_domains, n_ops, domains, ops, op_pp);
}

uint64_t msv_aln_item_bytes(uint32_t states_per_lane, uint64_t Le) {
    return msv_host::aln_item_bytes(states_per_lane, Le);
}

}  // extern "C"
