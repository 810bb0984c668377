// cal_host.cpp -- host-only half of the calibration stage (cal_host.h; msv.h "Calibration").
#include "cal_host.h"

#include <algorithm>
#include <cstring>
#include <limits>
#include <new>
#include <vector>

#include "host_cpu.h"
#include "msv_plan.h"

namespace msv_host {

CalThresholds cal_thresholds(const float* background) {
    double total = 0.0;
    for (int x = 0; x < 20; ++x) total += static_cast<double>(background[x]);
    CalThresholds T;
    double run = 0.0;
    for (int j = 0; j < kCalThresholds; ++j) {
        run += static_cast<double>(background[j]);
        T.t[j] = static_cast<uint32_t>(std::floor(16777216.0 * run / total));
    }
    return T;
}

uint64_t cal_chunk_sequences(uint64_t budget, uint64_t L) {
    if (L == 0) return 0;
    // cal_workspace_bytes(n, L) <= n (L + 8) + 23
    uint64_t n = budget > 23 ? (budget - 23) / (L + 8) : 0;
    n = std::min(n, (msvplan::kChunkBytes - 1) / L);
    return std::min(n, msvplan::kMaxLaunchSeqs - 1);
}

bool cal_plan(const msv_cal_options* options, uint32_t sets, CalPlan* plan) {
    msv_cal_options o;
    if (!read_sized(options, &o, sizeof(uint64_t))) return false;
    for (int s = 0; s < 3; ++s) {
        plan->n[s] = o.n[s] ? o.n[s] : kCalDefaultN[s];
        plan->L[s] = o.length[s] ? o.length[s] : kCalDefaultL[s];
        plan->scores[s] = o.scores[s];
        if (!(sets >> s & 1u)) continue;
        if (plan->n[s] < 2 || plan->n[s] >= (1ull << 40) || plan->L[s] >= (1ull << 31)) return false;
    }
    plan->tail = o.tail != 0.0 ? o.tail : kCalDefaultTail;
    plan->seed = o.seed_set ? o.seed : kCalDefaultSeed;
    plan->workspace = o.workspace_bytes ? o.workspace_bytes : kCalDefaultWorkspace;
    plan->insert_mode = o.insert_mode;
    return cal_tail_ok(plan->tail);
}

void cal_finish(const CalPlan& plan, uint32_t sets, double lambda, const msv_cal_fit* records, const uint64_t* chunks,
                float* stats, msv_cal_report* report) {
    msv_cal_report r;
    std::memset(&r, 0, sizeof(r));
    const double nan = std::numeric_limits<double>::quiet_NaN();
    r.ran = sets & 7u;
    r.lambda = lambda;
    r.gmu = r.glam = nan;
    for (int s = 0; s < 3; ++s) {
        r.location[s] = nan;
        r.n[s] = plan.n[s];
        r.length[s] = plan.L[s];
        if (!(sets >> s & 1u)) continue;
        r.location[s] = records[s].mu;
        r.chunks[s] = chunks[s];
        stats[2 * s] = static_cast<float>(records[s].mu);
        stats[2 * s + 1] = static_cast<float>(lambda);
        if (s == MSV_CAL_SET_FORWARD) {
            r.gmu = records[s].gmu;
            r.glam = records[s].glam;
            r.iterations = records[s].iterations;
        }
    }
    r.seed = plan.seed;
    r.tail = plan.tail;
    if (report && report->struct_size >= sizeof(uint32_t)) write_sized(report, r);
}

namespace {

// What every fit opens with: the bit scores as float64, their minimum, and the checks of msv.h.
msv_status bit_scores(const float* scores, uint64_t n, uint64_t L, std::vector<double>* y, double* xmin) {
    if (!scores || n < 2 || L >= (1ull << 40)) return MSV_ERR_INVALID_ARGUMENT;
    const float nullsc = L ? null1_score(L) : 0.0f;
    y->resize(n);
    double lo = std::numeric_limits<double>::infinity(), hi = -lo;
    for (uint64_t i = 0; i < n; ++i) {
        const double x = cal_bits(scores[i], L, nullsc);
        if (!cal_finite(scores[i]) || !cal_finite(x)) return MSV_ERR_INVALID_ARGUMENT;
        (*y)[i] = x;
        lo = std::min(lo, x);
        hi = std::max(hi, x);
    }
    if (!(hi > lo)) return MSV_ERR_INVALID_ARGUMENT;  // zero variance
    for (double& v : *y) v -= lo;
    *xmin = lo;
    return MSV_OK;
}

double sum_exp(const std::vector<double>& y, double lambda) {
    double S0 = 0.0;
    for (double v : y) S0 += std::exp(-lambda * v);
    return S0;
}

msv_status fit_gumbel(const float* scores, uint64_t n, uint64_t L, msv_cal_fit* out) {
    std::vector<double> y;
    double xmin = 0.0;
    const msv_status s = bit_scores(scores, n, L, &y, &xmin);
    if (s != MSV_OK) return s;
    double sum = 0.0;
    for (double v : y) sum += v;
    const double ybar = sum / static_cast<double>(n);
    double sq = 0.0;
    for (double v : y) sq += (v - ybar) * (v - ybar);
    const double var = sq / static_cast<double>(n - 1);
    const double lambda0 = 3.14159265358979323846 / std::sqrt(6.0 * var);
    double lambda = 0.0;
    const msv_status ns = cal_newton(
        ybar, lambda0,
        [&](double l, double* S) {
            S[0] = S[1] = S[2] = 0.0;
            for (double v : y) {
                const double e = std::exp(-l * v);
                S[0] += e;
                S[1] += v * e;
                S[2] += v * v * e;
            }
        },
        &lambda, &out->iterations);
    if (ns != MSV_OK) return ns;
    out->gmu = out->mu = cal_location(xmin, sum_exp(y, lambda), n, lambda);
    out->glam = out->lambda = lambda;
    return MSV_OK;
}

}  // namespace
}  // namespace msv_host

using namespace msv_host;

extern "C" {

msv_status msv_cal_lambda(const float* match_emissions, uint32_t model_length, const float* background,
                          double* lambda) {
    if (!match_emissions || !background || !lambda || model_length < 2) return MSV_ERR_INVALID_ARGUMENT;
    const uint32_t leng = model_length - 1;
    double H = 0.0;
    for (uint32_t k = 1; k <= leng; ++k)
        for (int x = 0; x < 20; ++x) {
            const double p = static_cast<double>(match_emissions[static_cast<size_t>(k) * 20 + x]);
            if (p > 0.0) H += p * std::log2(p / static_cast<double>(background[x]));
        }
    H /= static_cast<double>(leng);
    const double l = 0.69314718055994529 + 1.44 / (static_cast<double>(leng) * H);
    if (!cal_finite(l) || !(l > 0.0)) return MSV_ERR_INVALID_ARGUMENT;
    *lambda = l;
    return MSV_OK;
}

msv_status msv_cal_thresholds(const float* background, uint32_t* thresholds) {
    if (!background || !thresholds) return MSV_ERR_INVALID_ARGUMENT;
    const CalThresholds T = cal_thresholds(background);
    std::copy(T.t, T.t + kCalThresholds, thresholds);
    return MSV_OK;
}

msv_status msv_cal_codes_of_draws(const float* background, const uint32_t* draws, uint64_t n, uint8_t* codes) {
    if (!background || (n && (!draws || !codes))) return MSV_ERR_INVALID_ARGUMENT;
    const CalThresholds T = cal_thresholds(background);
    for (uint64_t i = 0; i < n; ++i) codes[i] = cal_code(T, draws[i]);
    return MSV_OK;
}

msv_status msv_cal_generate(const float* background, uint64_t seed, uint32_t set, uint64_t first, uint64_t n,
                            uint64_t L, uint8_t* codes, uint64_t* offsets) {
    if (!background || !offsets || (n && L && !codes) || L >= 0xffffffffull) return MSV_ERR_INVALID_ARGUMENT;
    if (L && n > std::numeric_limits<uint64_t>::max() / L) return MSV_ERR_INVALID_ARGUMENT;
    const CalThresholds T = cal_thresholds(background);
    for (uint64_t j = 0; j < n; ++j) {
        const uint64_t key = cal_key(seed, set, first + j);
        uint8_t* const row = codes + j * L;
        for (uint64_t i = 0; i < L; ++i) row[i] = cal_residue(T, key, static_cast<uint32_t>(i));
    }
    for (uint64_t j = 0; j <= n; ++j) offsets[j] = j * L;
    return MSV_OK;
}

msv_status msv_cal_fit_location(const float* scores, uint64_t n, uint64_t L, double lambda, double* mu) {
    if (!mu || !(lambda > 0.0) || !cal_finite(lambda)) return MSV_ERR_INVALID_ARGUMENT;
    std::vector<double> y;
    double xmin = 0.0;
    const msv_status s = bit_scores(scores, n, L, &y, &xmin);
    if (s != MSV_OK) return s;
    *mu = cal_location(xmin, sum_exp(y, lambda), n, lambda);
    return MSV_OK;
}

msv_status msv_cal_fit_gumbel(const float* scores, uint64_t n, uint64_t L, double* mu, double* lambda,
                              uint32_t* iterations) {
    if (!mu || !lambda) return MSV_ERR_INVALID_ARGUMENT;
    msv_cal_fit f{};
    const msv_status s = fit_gumbel(scores, n, L, &f);
    if (iterations) *iterations = f.iterations;
    if (s != MSV_OK) return s;
    *mu = f.gmu;
    *lambda = f.glam;
    return MSV_OK;
}

msv_status msv_cal_tau(double gmu, double glam, double lambda, double tail, double* tau) {
    if (!tau || !cal_tail_ok(tail) || !(glam > 0.0) || !(lambda > 0.0) || !cal_finite(gmu) || !cal_finite(glam) ||
        !cal_finite(lambda))
        return MSV_ERR_INVALID_ARGUMENT;
    *tau = cal_tau(gmu, glam, lambda, tail);
    return MSV_OK;
}

uint64_t msv_cal_workspace_bytes(uint64_t n, uint64_t L) { return cal_workspace_bytes(n, L); }

msv_status msv_cal_cpu_calibrate(const msv_hmm* hmm, uint32_t sets, const msv_cal_options* options, float* stats,
                                 msv_cal_report* report) try {
    if (!hmm || !stats || (sets & ~7u)) return MSV_ERR_INVALID_ARGUMENT;
    CalPlan plan;
    if (!cal_plan(options, sets, &plan)) return MSV_ERR_INVALID_ARGUMENT;
    const uint32_t M = static_cast<uint32_t>(msv_hmm_model_length(hmm));
    const float* const bg = msv_background_frequencies();
    double lambda = 0.0;
    msv_status s = msv_cal_lambda(msv_hmm_match_emissions(hmm), M, bg, &lambda);
    if (s != MSV_OK) return s;
    std::vector<float> msc(static_cast<size_t>(20) * M), isc(static_cast<size_t>(20) * M), tsc(static_cast<size_t>(7) * M);
    float b = 0, c = 0, j = 0;
    s = msv_hmm_viterbi_scores(hmm, plan.insert_mode, msc.data(), isc.data(), tsc.data(), &b, &c, &j);
    if (s != MSV_OK) return s;
    const float* const ins = plan.insert_mode == MSV_INSERTS_ZERO ? nullptr : isc.data();
    msv_cal_fit rec[3];
    uint64_t chunks[3] = {0, 0, 0};
    for (uint32_t set = 0; set < 3; ++set) {
        if (!(sets >> set & 1u)) continue;
        const uint64_t n = plan.n[set], L = plan.L[set];
        if (n > (1ull << 40) / L) return MSV_ERR_OUT_OF_MEMORY;  // the twin holds the whole sample
        std::vector<uint8_t> codes(n * L);
        std::vector<uint64_t> off(n + 1);
        s = msv_cal_generate(bg, plan.seed, set, 0, n, L, codes.data(), off.data());
        if (s != MSV_OK) return s;
        std::vector<float> sc(n);
        if (set == MSV_CAL_SET_FORWARD) {
            std::vector<double> d(n);
            s = msv_fwd_cpu_score_batch(msc.data(), ins, tsc.data(), M, b, c, j, codes.data(), off.data(), n, d.data());
            if (s != MSV_OK) return s;
            for (uint64_t q = 0; q < n; ++q) sc[q] = static_cast<float>(d[q]);
        } else {
            for (uint64_t q = 0; q < n; ++q) {
                const uint8_t* const row = codes.data() + q * L;
                if (set == MSV_CAL_SET_MSV) {
                    sc[q] = run_on_sequence(msc.data(), M, b, c, j, row, L);
                } else {
                    s = msv_vit_cpu_score(msc.data(), ins, tsc.data(), M, b, c, j, row, L, &sc[q]);
                    if (s != MSV_OK) return s;
                }
            }
        }
        if (plan.scores[set]) std::copy(sc.begin(), sc.end(), plan.scores[set]);
        std::memset(&rec[set], 0, sizeof(rec[set]));
        if (set == MSV_CAL_SET_FORWARD) {
            s = fit_gumbel(sc.data(), n, L, &rec[set]);
            if (s != MSV_OK) return s;
            rec[set].mu = cal_tau(rec[set].gmu, rec[set].glam, lambda, plan.tail);
            rec[set].lambda = lambda;
        } else {
            s = msv_cal_fit_location(sc.data(), n, L, lambda, &rec[set].mu);
            if (s != MSV_OK) return s;
        }
        chunks[set] = 1;
    }
    cal_finish(plan, sets, lambda, rec, chunks, stats, report);
    return MSV_OK;
} catch (const std::bad_alloc&) {
    return MSV_ERR_OUT_OF_MEMORY;
}

}  // extern "C"
