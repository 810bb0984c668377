// dom_host.cpp -- the domain stage on the host (msv.h states the model): the float64 Forward /
// Backward decode, the envelope rule, the kernel-layout Backward tables with the mirrored D-scan constants.  Host
// only, no HIP.
#include "dom_host.h"

#include <algorithm>
#include <cmath>
#include <limits>
#include <thread>

namespace msv_host {

namespace {

constexpr int kRows = 20;
constexpr int kArrays = 8;  // domk::kArrays: 7 own-node transition arrays + the D-scan suffix products
constexpr int kLanes = 64;
constexpr int kScanSteps = 6;
enum : int { B_MM = 0, B_MI = 1, B_MD = 2, B_IM = 3, B_II = 4, B_DM = 5, B_DD = 6, B_SFX = 7 };  // domk:: slot arrays
enum { MM, MI_, MD, IM, II_, DM, DD };  // file order m->m m->i m->d i->m i->i d->m d->d

inline double odds(float score) { return std::exp(static_cast<double>(score)); }  // exp(-inf) = 0

constexpr double kBig = 0x1p256, kDown = 0x1p-256;
constexpr double kLn2 = 0.69314718055994530942;

}  // namespace

void decode_run_on_sequence(const FwdModel& m, const uint8_t* codes, size_t L, double* fwd_score, double* bck_score,
                            double* begin, double* end, double* occ) {
    const double ninf = -std::numeric_limits<double>::infinity();
    if (L == 0) {
        if (fwd_score) *fwd_score = ninf;
        if (bck_score) *bck_score = ninf;
        return;
    }
    const size_t M = m.M, K = M - 1;
    float lf, mf;
    msv_sequence_transitions(L, &lf, &mf);
    const double loop = odds(lf), move = odds(mf);
    const double* xt = m.xt.data();

    // Forward, as forward_run_on_sequence, keeping every row's specials and exponent
    std::vector<double> fN(L + 1), fJ(L + 1), fC(L + 1), fB(L + 1), fE(L + 1);
    std::vector<int64_t> fe(L + 1);
    {
        std::vector<double> Mp(M, 0.0), Ip(M, 0.0), Dp(M, 0.0), Mc(M, 0.0), Ic(M, 0.0), Dc(M, 0.0);
        double N = 1.0, J = 0.0, C = 0.0, B = N * move;
        int64_t e2 = 0;
        fN[0] = N, fJ[0] = J, fC[0] = C, fB[0] = B, fE[0] = 0.0, fe[0] = 0;
        for (size_t i = 0; i < L; ++i) {
            const double* xm = m.xm.data() + static_cast<size_t>(codes[i]) * M;
            const double* xi = m.xi.data() + static_cast<size_t>(codes[i]) * M;
            const double Bt = B * m.tBM;
            double E = 0.0;
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
            Mp.swap(Mc);
            Ip.swap(Ic);
            Dp.swap(Dc);
            if (E > kBig) {
                for (size_t k = 1; k <= K; ++k) Mp[k] *= kDown, Ip[k] *= kDown, Dp[k] *= kDown;
                N *= kDown, J *= kDown, C *= kDown, B *= kDown, E *= kDown;
                e2 += 256;
            }
            fN[i + 1] = N, fJ[i + 1] = J, fC[i + 1] = C, fB[i + 1] = B, fE[i + 1] = E, fe[i + 1] = e2;
        }
    }
    const double Zs = fC[L] * move;  // Z = Zs 2^fe[L]
    if (fwd_score) *fwd_score = std::log(Zs) + static_cast<double>(fe[L]) * kLn2;

    // Backward: bM, bI of row i + 1 in Mn, In; the row's D chain in Dc (index K + 1: the 0 beyond the model)
    std::vector<double> Mn(M + 1, 0.0), In(M + 1, 0.0), Mc(M + 1, 0.0), Ic(M + 1, 0.0), Dc(M + 2, 0.0);
    std::vector<double> P(M + 1, 0.0), H(M + 1, 0.0);
    double bJ = 0.0, bC = 0.0, bN = 0.0;
    int64_t be = 0;  // the values are the true ones times 2^-be
    for (size_t i = L + 1; i-- > 0;) {
        double bB = 0.0;
        double lJ = 0.0, lC = 0.0, lN = 0.0;  // loop * the next row's specials, in this row's scale
        if (i == L) {
            std::fill(P.begin(), P.end(), 0.0);
            std::fill(H.begin(), H.end(), 0.0);
            bC = move;
            bJ = bN = 0.0;
        } else {
            const double* xm = m.xm.data() + static_cast<size_t>(codes[i]) * M;  // r = residue i + 1
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
            const double* t = xt + k * 7;  // node k (all 0 at node LENG)
            const double g = k < K ? P[k + 1] : 0.0, h = H[k];
            Dc[k] = (k >= 2 ? bE : 0.0) + t[DM] * g + t[DD] * Dc[k + 1];
            Mc[k] = bE + t[MM] * g + t[MI_] * h + t[MD] * Dc[k + 1];
            Ic[k] = t[IM] * g + t[II_] * h;
        }
        Mn.swap(Mc);
        In.swap(Ic);
        // the posteriors this row completes: end[i], begin[i + 1], occ[i + 1]
        const int sh = static_cast<int>(fe[i] + be - fe[L]);
        if (i >= 1 && end) end[i - 1] = std::ldexp(fE[i] * bE / Zs, sh);
        if (i < L) {
            if (begin) begin[i] = std::ldexp(fB[i] * bB / Zs, sh);
            if (occ) occ[i] = 1.0 - std::ldexp((fN[i] * lN + fJ[i] * lJ + fC[i] * lC) / Zs, sh);
        }
    }
    if (bck_score) *bck_score = std::log(bN) + static_cast<double>(be) * kLn2;
}

DomTables dom_tables(const float* msc, const float* isc_tab, const float* tsc, uint32_t model_length, int S,
                     bool isc) {
    DomTables t;
    t.fwd = fwd_tables(msc, isc_tab, tsc, model_length, S, isc);
    const int C2 = S / 2;
    const uint32_t K = model_length - 1;
    const size_t row2 = static_cast<size_t>(C2) * kLanes;
    auto f32 = [](double x) { return static_cast<float>(x); };
    t.bt.assign(2 * kArrays * row2, 0.0f);
    t.bscan.assign(kScanSteps * kLanes, 0.0f);
    auto at_slot = [&](int j, int l, int q) -> float& {
        return t.bt[2 * ((static_cast<size_t>(j) * C2 + q / 2) * kLanes + l) + (q & 1)];
    };
    static const int file_col[7] = {MM, MI_, MD, IM, II_, DM, DD};  // B_MM .. B_DD
    // the scan's multipliers are products of the float tDD odds the kernel reads, taken in float64
    double lane_prod[kLanes];
    for (int l = 0; l < kLanes; ++l) {
        double s = 1.0;
        for (int q = S - 1; q >= 0; --q) {
            const uint32_t k = static_cast<uint32_t>(l * S + q + 1);
            if (k >= 1 && k < K)  // nodes 1 .. LENG-1 have transitions
                for (int j = 0; j < 7; ++j) at_slot(j, l, q) = f32(odds(tsc[static_cast<size_t>(k) * 7 + file_col[j]]));
            s *= static_cast<double>(at_slot(B_DD, l, q));
            at_slot(B_SFX, l, q) = f32(s);
        }
        lane_prod[l] = s;
    }
    double a[kLanes], b[kLanes];
    std::copy(lane_prod, lane_prod + kLanes, a);
    for (int j = 0; j < kScanSteps; ++j) {
        for (int l = 0; l < kLanes; ++l) t.bscan[static_cast<size_t>(j) * kLanes + l] = f32(a[l]);
        for (int l = 0; l < kLanes; ++l) b[l] = l + (1 << j) < kLanes ? a[l] * a[l + (1 << j)] : a[l];
        std::copy(b, b + kLanes, a);
    }
    return t;
}

}  // namespace msv_host

extern "C" {

msv_status msv_dom_cpu_decode_batch(const float* match_scores, const float* insert_scores,
                                    const float* transition_scores, uint32_t model_length, float tr_B_Mk, float tr_E_C,
                                    float tr_E_J, const uint8_t* codes, const uint64_t* offsets, uint64_t n,
                                    double* fwd_scores, double* bck_scores, double* begin, double* end, double* occ) {
    if (!match_scores || !transition_scores || model_length < 2 || (n && !offsets)) return MSV_ERR_INVALID_ARGUMENT;
    if (n == 0) return MSV_OK;
    for (uint64_t s = 0; s < n; ++s)
        if (offsets[s + 1] < offsets[s]) return MSV_ERR_INVALID_ARGUMENT;
    if (offsets[n] > offsets[0] && !codes) return MSV_ERR_INVALID_ARGUMENT;
    for (uint64_t i = offsets[0]; i < offsets[n]; ++i)
        if (codes[i] >= 20) return MSV_ERR_BAD_RESIDUE;
    const msv_host::FwdModel m = msv_host::fwd_model(match_scores, insert_scores, transition_scores, model_length,
                                                     tr_B_Mk, tr_E_C, tr_E_J);
    const unsigned hw = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    const unsigned workers = static_cast<unsigned>(std::min<uint64_t>(hw, n));
    const uint64_t base = offsets[0];
    auto run = [&](unsigned w) {
        for (uint64_t s = w; s < n; s += workers) {
            const uint64_t o = offsets[s] - base;  // the per-residue outputs are indexed from the batch's first residue
            msv_host::decode_run_on_sequence(m, codes ? codes + offsets[s] : nullptr, offsets[s + 1] - offsets[s],
                                             fwd_scores ? fwd_scores + s : nullptr, bck_scores ? bck_scores + s : nullptr,
                                             begin ? begin + o : nullptr, end ? end + o : nullptr,
                                             occ ? occ + o : nullptr);
        }
    };
    if (workers <= 1) {
        run(0);
    } else {
        std::vector<std::thread> pool;
        for (unsigned w = 0; w < workers; ++w) pool.emplace_back(run, w);
        for (auto& t : pool) t.join();
    }
    return MSV_OK;
}

msv_status msv_dom_cpu_decode(const float* match_scores, const float* insert_scores, const float* transition_scores,
                              uint32_t model_length, float tr_B_Mk, float tr_E_C, float tr_E_J, const uint8_t* codes,
                              uint64_t L, double* fwd_score, double* bck_score, double* begin, double* end,
                              double* occ) {
    if (L && !codes) return MSV_ERR_INVALID_ARGUMENT;
    const uint64_t offsets[2] = {0, L};
    return msv_dom_cpu_decode_batch(match_scores, insert_scores, transition_scores, model_length, tr_B_Mk, tr_E_C,
                                    tr_E_J, codes, offsets, 1, fwd_score, bck_score, begin, end, occ);
}

msv_status msv_dom_regions(const float* begin, const float* end, const float* occ, uint64_t L, float rt1, float rt2,
                           uint32_t* n_regions, msv_dom_region* regions) {
    if (!n_regions || (L && (!begin || !end || !occ)) || L >= (1ull << 32)) return MSV_ERR_INVALID_ARGUMENT;
    uint32_t at = 0;
    *n_regions = msv_host::dom_regions_scan(begin, end, occ, L, rt1, rt2,
                                            [&](uint32_t i_from, uint32_t i_to, float nd, float mass) {
                                                if (regions) regions[at] = msv_dom_region{0, i_from, i_to, nd, mass};
                                                ++at;
                                            });
    return MSV_OK;
}

msv_status msv_dom_scan_constants(const float* transition_scores, uint32_t model_length, uint32_t states_per_lane,
                                  float* slot_dd, float* slot_suffix, float* step_products) {
    const uint32_t S = states_per_lane;
    if (!transition_scores || model_length < 2 || S < 2 || S % 2 || S > 64 ||
        static_cast<uint64_t>(S) * 64 < model_length - 1)
        return MSV_ERR_INVALID_ARGUMENT;
    std::vector<float> msc(static_cast<size_t>(20) * model_length, 0.0f);
    const msv_host::DomTables t =
        msv_host::dom_tables(msc.data(), nullptr, transition_scores, model_length, static_cast<int>(S), false);
    const size_t C2 = S / 2;
    for (uint32_t l = 0; l < 64; ++l)
        for (uint32_t q = 0; q < S; ++q) {
            const size_t in_array = 2 * ((q / 2) * 64 + l) + (q & 1);
            if (slot_dd) slot_dd[l * S + q] = t.bt[2 * 6 * C2 * 64 + in_array];
            if (slot_suffix) slot_suffix[l * S + q] = t.bt[2 * 7 * C2 * 64 + in_array];
        }
    if (step_products) std::copy(t.bscan.begin(), t.bscan.end(), step_products);
    return MSV_OK;
}

uint64_t msv_dom_sequence_bytes(uint64_t L) { return msv_host::dom_sequence_bytes(L); }

}  // extern "C"
