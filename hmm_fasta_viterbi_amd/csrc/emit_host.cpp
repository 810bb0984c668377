// emit_host.cpp -- host-only half of the emit stage (emit_host.h; msv.h "Emit stage").
#include "emit_host.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <memory>
#include <new>

#include "host_cpu.h"

namespace msv_host {

namespace {

// T[j] = floor(2^24 (w[0] + .. + w[j]) / total), j < c - 1: msv_cal_thresholds' rule.  false: no total.
bool thresholds(const double* w, int c, uint32_t* T) {
    double total = 0.0;
    for (int x = 0; x < c; ++x) total += w[x];
    if (!(total > 0.0) || !std::isfinite(total)) return false;
    double run = 0.0;
    for (int j = 0; j + 1 < c; ++j) {
        run += w[j];
        T[j] = static_cast<uint32_t>(std::floor(16777216.0 * run / total));
    }
    return true;
}

bool row_thresholds(const float* p, int c, uint32_t* T) {
    double w[20];
    for (int x = 0; x < c; ++x) w[x] = static_cast<double>(p[x]);
    return thresholds(w, c, T);
}

// A sink that appends to a result.
struct VectorSink {
    msv_emit_result* r;
    uint32_t seq;
    void residue(uint32_t code) { r->codes.push_back(static_cast<uint8_t>(code)); }
    void op(uint32_t c) { r->ops.push_back(static_cast<uint8_t>(c)); }
    void domain(uint32_t i_from, uint32_t i_to, uint32_t k_from, uint32_t k_to, uint32_t len) {
        msv_vit_domain d;
        d.seq = seq;
        d.i_from = i_from;
        d.i_to = i_to;
        d.k_from = k_from;
        d.k_to = k_to;
        d.ops_len = len;
        d.ops_begin = r->ops.size() - len;
        r->domains.push_back(d);
    }
};

}  // namespace

msv_status emit_tables(const msv_hmm* hmm, const msv_emit_options* options, EmitTables* out) {
    if (!hmm || !out) return MSV_ERR_INVALID_ARGUMENT;
    msv_emit_options o;
    if (!read_sized(options, &o, sizeof(uint64_t))) return MSV_ERR_INVALID_ARGUMENT;
    const uint64_t Lc = o.length_set ? o.length : kEmitDefaultLength;
    const uint64_t max_length = o.max_length ? o.max_length : kEmitDefaultMaxLength;
    if (Lc >= (1ull << 40) || max_length >= (1ull << 31) || (o.unihit != 0 && o.unihit != 1) ||
        (o.insert_mode != MSV_INSERTS_ZERO && o.insert_mode != MSV_INSERTS_LOG_ODDS))
        return MSV_ERR_INVALID_ARGUMENT;
    const size_t M = msv_hmm_model_length(hmm);
    if (M < 2 || M - 1 > kEmitMaxLeng) return MSV_ERR_INVALID_ARGUMENT;
    const uint32_t leng = static_cast<uint32_t>(M - 1);

    EmitConfig& c = out->config;
    std::memset(&c, 0, sizeof(c));
    if (!row_thresholds(msv_background_frequencies(), 20, c.bg)) return MSV_ERR_INVALID_ARGUMENT;
    const double loop[2] = {static_cast<double>(Lc), 3.0};
    if (!thresholds(loop, 2, &c.t_loop)) return MSV_ERR_INVALID_ARGUMENT;
    const double ej[2] = {1.0, 1.0};  // nu = 2
    if (!o.unihit && !thresholds(ej, 2, &c.t_j)) return MSV_ERR_INVALID_ARGUMENT;
    c.leng = leng;
    c.max_length = static_cast<uint32_t>(max_length);
    c.multihit = o.unihit ? 0u : 1u;
    c.file_inserts = o.insert_mode == MSV_INSERTS_LOG_ODDS ? 1u : 0u;

    out->model_length = static_cast<uint32_t>(M);
    out->length = Lc;
    out->match.assign(M * kEmitThresholds, 0u);
    out->insert.assign(M * kEmitThresholds, 0u);
    out->trans.assign(M * 4, 0u);
    const float* const mat = msv_hmm_match_emissions(hmm);
    const float* const ins = msv_hmm_insert_emissions(hmm);
    const float* const tr = msv_hmm_transitions(hmm);
    enum { MM, MI, MD, IM, II, DM, DD };
    for (uint32_t k = 1; k <= leng; ++k) {
        uint32_t* const mrow = &out->match[static_cast<size_t>(k) * kEmitThresholds];
        if (!row_thresholds(mat + static_cast<size_t>(k) * 20, 20, mrow)) return MSV_ERR_INVALID_ARGUMENT;
        if (k == leng) break;  // nodes 1 .. LENG-1 have an insert state and successors
        uint32_t* const irow = &out->insert[static_cast<size_t>(k) * kEmitThresholds];
        if (c.file_inserts) {
            if (!row_thresholds(ins + static_cast<size_t>(k) * 20, 20, irow)) return MSV_ERR_INVALID_ARGUMENT;
        } else {
            std::copy(c.bg, c.bg + kEmitThresholds, irow);
        }
        const float* const t = tr + static_cast<size_t>(k) * 7;
        uint32_t* const T = &out->trans[static_cast<size_t>(k) * 4];
        const double m[3] = {static_cast<double>(t[MM]), static_cast<double>(t[MI]), static_cast<double>(t[MD])};
        const double i[2] = {static_cast<double>(t[IM]), static_cast<double>(t[II])};
        const double d[2] = {static_cast<double>(t[DM]), static_cast<double>(t[DD])};
        if (!thresholds(m, 3, T) || !thresholds(i, 2, T + 2) || !thresholds(d, 2, T + 3))
            return MSV_ERR_INVALID_ARGUMENT;
    }
    return MSV_OK;
}

}  // namespace msv_host

using namespace msv_host;

extern "C" {

msv_status msv_emit_tables(const msv_hmm* hmm, const msv_emit_options* options, uint32_t* background, uint32_t* match,
                           uint32_t* insert, uint32_t* transitions, uint32_t* specials) try {
    EmitTables t;
    const msv_status s = emit_tables(hmm, options, &t);
    if (s != MSV_OK) return s;
    if (background) std::copy(t.config.bg, t.config.bg + kEmitThresholds, background);
    if (match) std::copy(t.match.begin(), t.match.end(), match);
    if (insert) std::copy(t.insert.begin(), t.insert.end(), insert);
    if (transitions) std::copy(t.trans.begin(), t.trans.end(), transitions);
    if (specials) {
        specials[0] = t.config.t_loop;
        specials[1] = t.config.t_j;
    }
    return MSV_OK;
} catch (const std::bad_alloc&) {
    return MSV_ERR_OUT_OF_MEMORY;
}

msv_status msv_emit_generate(const msv_hmm* hmm, const msv_emit_options* options, uint64_t seed, uint64_t first,
                             uint64_t n, msv_emit_result** result) try {
    if (!result) return MSV_ERR_INVALID_ARGUMENT;
    *result = nullptr;
    if (n >= (1ull << 32)) return MSV_ERR_INVALID_ARGUMENT;
    EmitTables t;
    const msv_status s = emit_tables(hmm, options, &t);
    if (s != MSV_OK) return s;
    std::unique_ptr<msv_emit_result> guard(new msv_emit_result);
    msv_emit_result* const r = guard.get();
    r->offsets.assign(n + 1, 0);
    r->domain_offsets.assign(n + 1, 0);
    r->truncated.assign(n, 0);
    for (uint64_t j = 0; j < n; ++j) {
        VectorSink sink{r, static_cast<uint32_t>(j)};
        const EmitCounts c =
            emit_walk(t.config, t.match.data(), t.insert.data(), t.trans.data(), emit_key(seed, first + j), sink);
        r->truncated[j] = static_cast<uint8_t>(c.truncated);
        r->offsets[j + 1] = r->codes.size();
        r->domain_offsets[j + 1] = r->domains.size();
    }
    *result = guard.release();
    return MSV_OK;
} catch (const std::bad_alloc&) {
    return MSV_ERR_OUT_OF_MEMORY;
}

uint64_t msv_emit_result_count(const msv_emit_result* r) { return r ? r->truncated.size() : 0; }
uint64_t msv_emit_result_residues(const msv_emit_result* r) { return r ? r->codes.size() : 0; }
uint64_t msv_emit_result_domains(const msv_emit_result* r) { return r ? r->domains.size() : 0; }
uint64_t msv_emit_result_ops(const msv_emit_result* r) { return r ? r->ops.size() : 0; }
uint64_t msv_emit_result_chunks(const msv_emit_result* r) { return r ? r->chunks : 0; }

msv_status msv_emit_result_copy(const msv_emit_result* r, uint8_t* codes, uint64_t* offsets, uint64_t* domain_offsets,
                                msv_vit_domain* domains, uint8_t* ops, uint8_t* truncated) {
    if (!r) return MSV_ERR_INVALID_ARGUMENT;
    if (codes) std::copy(r->codes.begin(), r->codes.end(), codes);
    if (offsets) std::copy(r->offsets.begin(), r->offsets.end(), offsets);
    if (domain_offsets) std::copy(r->domain_offsets.begin(), r->domain_offsets.end(), domain_offsets);
    if (domains) std::copy(r->domains.begin(), r->domains.end(), domains);
    if (ops) std::copy(r->ops.begin(), r->ops.end(), ops);
    if (truncated) std::copy(r->truncated.begin(), r->truncated.end(), truncated);
    return MSV_OK;
}

void msv_emit_result_free(msv_emit_result* r) { delete r; }

msv_status msv_emit_path_score(const float* msc, const float* isc, const float* tsc, uint32_t M, float tr_B_Mk,
                               float tr_E_C, float tr_E_J, const uint8_t* codes, uint64_t L,
                               const msv_vit_domain* domains, uint32_t n_domains, const uint8_t* ops, double* score) {
    if (!msc || !tsc || !score || M < 2 || (L && !codes) || (n_domains && (!domains || !ops)))
        return MSV_ERR_INVALID_ARGUMENT;
    for (uint64_t i = 0; i < L; ++i)
        if (codes[i] >= 20) return MSV_ERR_BAD_RESIDUE;
    if (n_domains == 0) {
        *score = -std::numeric_limits<double>::infinity();
        return MSV_OK;
    }
    enum { MM, MI, MD, IM, II, DM, DD };
    const uint32_t leng = M - 1;
    float loop, move;
    msv_sequence_transitions(L, &loop, &move);
    double sc = 0.0;
    uint64_t inside = 0, last_to = 0;
    for (uint32_t q = 0; q < n_domains; ++q) {
        const msv_vit_domain& d = domains[q];
        if (d.i_from < 1 || d.i_from > d.i_to || d.i_to > L || d.i_from <= last_to || d.k_from < 1 ||
            d.k_from > d.k_to || d.k_to > leng || d.ops_len == 0)
            return MSV_ERR_INVALID_ARGUMENT;
        const uint8_t* const o = ops + d.ops_begin;
        uint64_t i = d.i_from - 1;
        uint32_t k = d.k_from - 1;
        uint8_t prev = 0;
        sc += static_cast<double>(tr_B_Mk);
        for (uint32_t x = 0; x < d.ops_len; ++x) {
            const uint8_t op = o[x];
            if (op == 'M') {
                ++i;
                ++k;
                if (i > d.i_to || k > d.k_to) return MSV_ERR_INVALID_ARGUMENT;
                const int into = prev == 'M' ? MM : prev == 'I' ? IM : DM;
                if (prev) sc += static_cast<double>(tsc[static_cast<size_t>(k - 1) * 7 + into]);
                sc += static_cast<double>(msc[static_cast<size_t>(codes[i - 1]) * M + k]);
            } else if (op == 'I') {
                ++i;
                if ((prev != 'M' && prev != 'I') || i > d.i_to || k >= leng) return MSV_ERR_INVALID_ARGUMENT;
                sc += static_cast<double>(tsc[static_cast<size_t>(k) * 7 + (prev == 'M' ? MI : II)]);
                if (isc) sc += static_cast<double>(isc[static_cast<size_t>(codes[i - 1]) * M + k]);
            } else if (op == 'D') {
                ++k;
                if ((prev != 'M' && prev != 'D') || k > d.k_to) return MSV_ERR_INVALID_ARGUMENT;
                sc += static_cast<double>(tsc[static_cast<size_t>(k - 1) * 7 + (prev == 'M' ? MD : DD)]);
            } else {
                return MSV_ERR_INVALID_ARGUMENT;
            }
            prev = op;
        }
        if (i != d.i_to || k != d.k_to) return MSV_ERR_INVALID_ARGUMENT;
        sc += static_cast<double>(q + 1 == n_domains ? tr_E_C : tr_E_J);
        inside += d.i_to - d.i_from + 1;
        last_to = d.i_to;
    }
    sc += static_cast<double>(L - inside) * static_cast<double>(loop);
    sc += (static_cast<double>(n_domains) + 1.0) * static_cast<double>(move);
    *score = sc;
    return MSV_OK;
}

uint64_t msv_emit_workspace_bytes(uint64_t n, uint64_t residues, uint64_t domains, uint64_t ops, int truth) {
    return emit_workspace_bytes(n, residues, domains, ops, truth != 0);
}

}  // extern "C"
