// bias_filter_host.cpp -- the bias filter's host half (bias_filter_host.h) and its host-only C-ABI entry points
// (msv.h "Bias filter"): the float64 definition, its batch form, the filtered P-values and the device table.
#include "bias_filter_host.h"

#include <cmath>
#include <limits>

namespace msv_host {

msv_status bf_model(const float* compo, const float* background, uint32_t model_length, BfModel* out) {
    if (!compo || !background || !out || model_length < 2) return MSV_ERR_INVALID_ARGUMENT;
    BfModel m;
    for (int x = 0; x < 20; ++x) {
        if (!std::isfinite(compo[x]) || compo[x] < 0.0f) return MSV_ERR_INVALID_ARGUMENT;
        if (!std::isfinite(background[x]) || !(background[x] > 0.0f)) return MSV_ERR_INVALID_ARGUMENT;
        m.r[x] = static_cast<double>(compo[x]) / static_cast<double>(background[x]);
    }
    const double L0 = 400.0f, L1 = static_cast<float>(model_length - 1) / 8.0f;
    m.t00 = L0 / (L0 + 1.0);
    m.t01 = 1.0 / (L0 + 1.0);
    m.t10 = 1.0 / (L1 + 1.0);
    m.t11 = L1 / (L1 + 1.0);
    m.pi0 = 0.999;
    m.pi1 = 0.001;
    *out = m;
    return MSV_OK;
}

double bf_score(const BfModel& m, const uint8_t* codes, size_t L, bool* bad) {
    *bad = false;
    if (L == 0) return 0.0;
    double v0 = m.pi0, v1 = m.pi1;
    long long scale = 0;  // the row is v * 2^scale
    for (size_t i = 0; i < L; ++i) {
        const uint8_t x = codes[i];
        if (x >= 20) {
            *bad = true;
            return std::numeric_limits<double>::quiet_NaN();
        }
        double n0 = v0, n1 = v1;
        if (i) {
            n0 = v0 * m.t00 + v1 * m.t10;
            n1 = v0 * m.t01 + v1 * m.t11;
        }
        n1 *= m.r[x];
        const double top = n0 > n1 ? n0 : n1;
        if (!(top > 0.0)) return -std::numeric_limits<double>::infinity();  // (every path has odds 0)
        int e = 0;
        (void)std::frexp(top, &e);
        v0 = std::ldexp(n0, -e);
        v1 = std::ldexp(n1, -e);
        scale += e;
    }
    return std::log(v0 + v1) + static_cast<double>(scale) * 0.69314718055994530942;
}

msv_status bf_device_table(const BfModel& m, float* table) {
    if (!table) return MSV_ERR_INVALID_ARGUMENT;
    const double t[6] = {m.t00, m.t01, m.t10, m.t11, m.pi0, m.pi1};
    for (int k = 0; k < 6; ++k) table[k] = static_cast<float>(t[k]);
    for (int x = 0; x < 20; ++x) {
        const float r = static_cast<float>(m.r[x]);
        if (!(r >= 0x1p-24f && r <= 0x1p7f)) return MSV_ERR_UNSUPPORTED_MODEL;
        table[kBfTableR + x] = r;
    }
    return MSV_OK;
}

}  // namespace msv_host

extern "C" {

msv_status msv_bf_cpu_score(const float* compo, const float* background, uint32_t model_length, const uint8_t* codes,
                            uint64_t L, double* bias) {
    if (!bias || (L && !codes)) return MSV_ERR_INVALID_ARGUMENT;
    msv_host::BfModel m;
    const msv_status s = msv_host::bf_model(compo, background, model_length, &m);
    if (s != MSV_OK) return s;
    bool bad = false;
    *bias = msv_host::bf_score(m, codes, L, &bad);
    return bad ? MSV_ERR_BAD_RESIDUE : MSV_OK;
}

msv_status msv_bf_cpu_score_batch(const float* compo, const float* background, uint32_t model_length,
                                  const uint8_t* codes, const uint64_t* offsets, uint64_t n, double* bias) {
    if (n && (!offsets || !bias)) return MSV_ERR_INVALID_ARGUMENT;
    msv_host::BfModel m;
    const msv_status s = msv_host::bf_model(compo, background, model_length, &m);
    if (s != MSV_OK) return s;
    bool any_bad = false;
    for (uint64_t i = 0; i < n; ++i) {
        if (offsets[i + 1] < offsets[i]) return MSV_ERR_INVALID_ARGUMENT;
        const uint64_t L = offsets[i + 1] - offsets[i];
        if (L && !codes) return MSV_ERR_INVALID_ARGUMENT;
        bool bad = false;
        bias[i] = msv_host::bf_score(m, L ? codes + offsets[i] : nullptr, L, &bad);
        any_bad = any_bad || bad;
    }
    return any_bad ? MSV_ERR_BAD_RESIDUE : MSV_OK;
}

msv_status msv_bf_pvalues(const float* scores, const float* bias, const uint64_t* offsets, uint64_t n, float location,
                          float scale, int kind, double* pvalues) {
    if (n && (!scores || !bias || !offsets || !pvalues)) return MSV_ERR_INVALID_ARGUMENT;
    if (kind != MSV_BF_GUMBEL && kind != MSV_BF_EXPONENTIAL) return MSV_ERR_INVALID_ARGUMENT;
    for (uint64_t i = 0; i < n; ++i) {
        if (offsets[i + 1] < offsets[i]) return MSV_ERR_INVALID_ARGUMENT;
        const uint64_t L = offsets[i + 1] - offsets[i];
        pvalues[i] = kind == MSV_BF_GUMBEL ? msv_host::bf_gumbel_pvalue(scores[i], bias[i], L, location, scale)
                                           : msv_host::bf_exponential_pvalue(scores[i], bias[i], L, location, scale);
    }
    return MSV_OK;
}

msv_status msv_bf_device_table(const float* compo, const float* background, uint32_t model_length, float* table) {
    msv_host::BfModel m;
    const msv_status s = msv_host::bf_model(compo, background, model_length, &m);
    return s != MSV_OK ? s : msv_host::bf_device_table(m, table);
}

}  // extern "C"
