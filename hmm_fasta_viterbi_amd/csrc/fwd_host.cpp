// fwd_host.cpp -- the Forward stage on the host (msv.h states the model): the float64 reference
// DP, the kernel-layout odds tables with the D-scan constants, and the P-values.  Host only, no HIP.
#include "fwd_host.h"

#include <algorithm>
#include <limits>
#include <thread>

namespace msv_host {

namespace {

constexpr int kRows = 20;
constexpr int kArrays = 8;  // fwdk::kArrays: 7 transition arrays + the D-scan prefix products
constexpr int kLanes = 64;
constexpr int kScanSteps = 6;
enum : int { MM_IN = 0, IM_IN = 1, DM_IN = 2, MI = 3, II = 4, MD_IN = 5, DD_IN = 6, DC = 7 };  // fwdk:: slot arrays
enum { MM, MI_, MD, IM, II_, DM, DD };  // file order m->m m->i m->d i->m i->i d->m d->d

inline double odds(float score) { return std::exp(static_cast<double>(score)); }  // exp(-inf) = 0

}  // namespace

FwdModel fwd_model(const float* msc, const float* isc, const float* tsc, size_t M, float tr_B_Mk, float tr_E_C,
                   float tr_E_J) {
    FwdModel m;
    m.M = M;
    m.xm.assign(kRows * M, 0.0);
    m.xi.assign(kRows * M, 1.0);
    m.xt.assign(7 * M, 0.0);
    for (size_t r = 0; r < kRows; ++r)
        for (size_t k = 1; k < M; ++k) {
            m.xm[r * M + k] = odds(msc[r * M + k]);
            if (isc) m.xi[r * M + k] = odds(isc[r * M + k]);
        }
    for (size_t k = 1; k + 1 < M; ++k)  // nodes 1 .. LENG-1: node 0 enters through tBM, node LENG has no successor
        for (int t = 0; t < 7; ++t) m.xt[k * 7 + t] = odds(tsc[k * 7 + t]);
    m.tBM = odds(tr_B_Mk);
    m.tEC = odds(tr_E_C);
    m.tEJ = odds(tr_E_J);
    return m;
}

double forward_run_on_sequence(const FwdModel& m, const uint8_t* codes, size_t L) {
    if (L == 0) return -std::numeric_limits<double>::infinity();
    const size_t M = m.M, K = M - 1;
    float lf, mf;
    msv_sequence_transitions(L, &lf, &mf);
    const double loop = odds(lf), move = odds(mf);
    std::vector<double> Mp(M, 0.0), Ip(M, 0.0), Dp(M, 0.0), Mc(M, 0.0), Ic(M, 0.0), Dc(M, 0.0);
    double N = 1.0, J = 0.0, C = 0.0, B = N * move;
    int64_t e2 = 0;  // the values are the true ones times 2^-e2
    constexpr double kBig = 0x1p256, kDown = 0x1p-256;
    const double* xt = m.xt.data();
    for (size_t i = 0; i < L; ++i) {
        const double* xm = m.xm.data() + static_cast<size_t>(codes[i]) * M;
        const double* xi = m.xi.data() + static_cast<size_t>(codes[i]) * M;
        const double Bt = B * m.tBM;
        double E = 0.0;
        for (size_t k = 1; k <= K; ++k) {
            const double* tin = xt + (k - 1) * 7;  // node k-1 (all 0 at node 0)
            const double* tout = xt + k * 7;       // node k (all 0 at node LENG)
            Mc[k] = xm[k] * (Mp[k - 1] * tin[MM] + Ip[k - 1] * tin[IM] + Dp[k - 1] * tin[DM] + Bt);
            Ic[k] = xi[k] * (Mp[k] * tout[MI_] + Ip[k] * tout[II_]);
            Dc[k] = Mc[k - 1] * tin[MD] + Dc[k - 1] * tin[DD];
            E += Mc[k] + Dc[k];  // local exits from M_k and (k >= 2; D_1 is 0) from D_k
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
            N *= kDown, J *= kDown, C *= kDown, B *= kDown;
            e2 += 256;
        }
    }
    return std::log(C * move) + static_cast<double>(e2) * 0.69314718055994530942;
}

FwdTables fwd_tables(const float* msc, const float* isc_tab, const float* tsc, uint32_t model_length, int S,
                     bool isc) {
    const int C2 = S / 2;
    const uint32_t M = model_length, K = M - 1;
    const size_t row2 = static_cast<size_t>(C2) * kLanes;
    auto state = [&](int l, int q) -> uint32_t { return static_cast<uint32_t>(l * S + q + 1); };
    auto f32 = [](double x) { return static_cast<float>(x); };
    FwdTables t;
    t.et.assign(2 * kRows * row2, 0.0f);
    t.it.assign(isc ? 2 * kRows * row2 : 0, 1.0f);
    t.tt.assign(2 * kArrays * row2, 0.0f);
    t.scan.assign(kScanSteps * kLanes, 0.0f);
    for (int r = 0; r < kRows; ++r)
        for (int c = 0; c < C2; ++c)
            for (int l = 0; l < kLanes; ++l)
                for (int h = 0; h < 2; ++h) {
                    const uint32_t k = state(l, 2 * c + h);
                    const size_t at = 2 * ((static_cast<size_t>(r) * C2 + c) * kLanes + l) + h;
                    if (k <= K) t.et[at] = f32(odds(msc[static_cast<size_t>(r) * M + k]));
                    if (isc && k < K) t.it[at] = f32(odds(isc_tab[static_cast<size_t>(r) * M + k]));
                }
    auto slot_t = [&](int j, uint32_t k) -> float {
        if (k > K) return 0.0f;  // padding slots
        const float* tin = tsc + static_cast<size_t>(k - 1) * 7;  // node k-1 -> node k
        const float* tout = tsc + static_cast<size_t>(k) * 7;     // node k -> I(k)
        switch (j) {
            case MM_IN: return k >= 2 ? f32(odds(tin[MM])) : 0.0f;
            case IM_IN: return k >= 2 ? f32(odds(tin[IM])) : 0.0f;
            case DM_IN: return k >= 2 ? f32(odds(tin[DM])) : 0.0f;
            case MI: return k < K ? f32(odds(tout[MI_])) : 0.0f;
            case II: return k < K ? f32(odds(tout[II_])) : 0.0f;
            case MD_IN: return k >= 2 ? f32(odds(tin[MD])) : 0.0f;
            case DD_IN: return k >= 2 ? f32(odds(tin[DD])) : 0.0f;
        }
        return 0.0f;
    };
    auto at_slot = [&](int j, int l, int q) -> float& {
        return t.tt[2 * ((static_cast<size_t>(j) * C2 + q / 2) * kLanes + l) + (q & 1)];
    };
    // the scan's multipliers are products of the float tDD odds the kernel reads, taken in float64
    double lane_prod[kLanes];
    for (int l = 0; l < kLanes; ++l) {
        double c = 1.0;
        for (int q = 0; q < S; ++q) {
            for (int j = 0; j < 7; ++j) at_slot(j, l, q) = slot_t(j, state(l, q));
            c *= static_cast<double>(at_slot(DD_IN, l, q));
            at_slot(DC, l, q) = f32(c);
        }
        lane_prod[l] = c;
    }
    double a[kLanes], b[kLanes];
    std::copy(lane_prod, lane_prod + kLanes, a);
    for (int j = 0; j < kScanSteps; ++j) {
        for (int l = 0; l < kLanes; ++l) t.scan[static_cast<size_t>(j) * kLanes + l] = f32(a[l]);
        for (int l = 0; l < kLanes; ++l) b[l] = l >= (1 << j) ? a[l] * a[l - (1 << j)] : a[l];
        std::copy(b, b + kLanes, a);
    }
    return t;
}

}  // namespace msv_host

extern "C" {

msv_status msv_fwd_cpu_score_batch(const float* match_scores, const float* insert_scores,
                                   const float* transition_scores, uint32_t model_length, float tr_B_Mk, float tr_E_C,
                                   float tr_E_J, const uint8_t* codes, const uint64_t* offsets, uint64_t n,
                                   double* scores) {
    if (!match_scores || !transition_scores || model_length < 2 || (n && (!offsets || !scores)))
        return MSV_ERR_INVALID_ARGUMENT;
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
    auto run = [&](unsigned w) {
        for (uint64_t s = w; s < n; s += workers)
            scores[s] = msv_host::forward_run_on_sequence(m, codes ? codes + offsets[s] : nullptr,
                                                          offsets[s + 1] - offsets[s]);
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

msv_status msv_fwd_cpu_score(const float* match_scores, const float* insert_scores, const float* transition_scores,
                             uint32_t model_length, float tr_B_Mk, float tr_E_C, float tr_E_J, const uint8_t* codes,
                             uint64_t L, double* score) {
    if (!score || (L && !codes)) return MSV_ERR_INVALID_ARGUMENT;
    const uint64_t offsets[2] = {0, L};
    return msv_fwd_cpu_score_batch(match_scores, insert_scores, transition_scores, model_length, tr_B_Mk, tr_E_C,
                                   tr_E_J, codes, offsets, 1, score);
}

msv_status msv_fwd_pvalues(const float* scores, const uint64_t* offsets, uint64_t n, float tau, float lambda,
                           double* pvalues) {
    if (n && (!scores || !offsets || !pvalues)) return MSV_ERR_INVALID_ARGUMENT;
    for (uint64_t i = 0; i < n; ++i) {
        if (offsets[i + 1] < offsets[i]) return MSV_ERR_INVALID_ARGUMENT;
        pvalues[i] = msv_host::fwd_pvalue_of(scores[i], offsets[i + 1] - offsets[i], tau, lambda);
    }
    return MSV_OK;
}

msv_status msv_fwd_scan_constants(const float* transition_scores, uint32_t model_length, uint32_t states_per_lane,
                                  float* slot_dd, float* slot_prefix, float* step_products) {
    const uint32_t S = states_per_lane;
    if (!transition_scores || model_length < 2 || S < 2 || S % 2 || S > 64 ||
        static_cast<uint64_t>(S) * 64 < model_length - 1)
        return MSV_ERR_INVALID_ARGUMENT;
    std::vector<float> msc(static_cast<size_t>(20) * model_length, 0.0f);
    const msv_host::FwdTables t =
        msv_host::fwd_tables(msc.data(), nullptr, transition_scores, model_length, static_cast<int>(S), false);
    const size_t C2 = S / 2;
    for (uint32_t l = 0; l < 64; ++l)
        for (uint32_t q = 0; q < S; ++q) {
            const size_t in_array = 2 * ((q / 2) * 64 + l) + (q & 1);
            if (slot_dd) slot_dd[l * S + q] = t.tt[2 * 6 * C2 * 64 + in_array];
            if (slot_prefix) slot_prefix[l * S + q] = t.tt[2 * 7 * C2 * 64 + in_array];
        }
    if (step_products) std::copy(t.scan.begin(), t.scan.end(), step_products);
    return MSV_OK;
}

}  // extern "C"
