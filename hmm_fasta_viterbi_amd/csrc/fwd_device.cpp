// fwd_device.cpp -- C-ABI of the Forward stage (msv.h) on the HIP runtime.
//
// A msv_fwd_profile is a stage profile (stage_profile.h: tables, length table, launch slots, streams, error
// words) of one compiled variant of fwd_kernel.hip, with odds tables, the D-scan constants and an odds {loop, move}
// table; a batch -- typically the Viterbi filter's survivors, selected on the device -- is one persistent launch.
// The entry points are their argument checks and one call into stage_profile.h; what is only the Forward stage's
// stands here.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "bias_filter_device.h"
#include "fwd_host.h"
#include "fwd_kernel.h"
#include "hip_rt.h"
#include "msv.h"
#include "msv_kernel.h"
#include "stage_profile.h"

using msvrt::csr_extent;
using msvrt::DeviceBuffer;
using msvrt::DeviceGuard;
using msvrt::hip_status;
using stagedev::kHostErrWord;

// The shared stage profile with the odds constants, the variant and its scan constants, and
// msv_fwd_filter_batch's buffers: the MSV and Viterbi scores, the two survivor lists (their counts:
// stagedev::kSelWord, kSel2Word) and the P-values.
struct msv_fwd_profile : stagedev::StageProfile {
    float tBM = 0, tEC = 0, tEJ = 0;  // odds of tr_B_Mk, tr_E_C, tr_E_J
    const fwdk::FwdVariant* v = nullptr;
    DeviceBuffer<float> d_scan;
    DeviceBuffer<float> d_msv_out, d_vit_out;
    DeviceBuffer<uint32_t> d_sel1, d_sel2;
    DeviceBuffer<double> d_pv;
};

namespace {

float odds(float log_score) { return static_cast<float>(std::exp(static_cast<double>(log_score))); }

// Lays the variant's tables out (msv_host::fwd_tables) and uploads them, all or none.
msv_status install(msv_fwd_profile* p, const fwdk::FwdVariant* v) {
    const msv_host::FwdTables t =
        msv_host::fwd_tables(p->msc.data(), p->isc_tab.data(), p->tsc.data(), p->model_length, v->S, p->isc);
    DeviceBuffer<float2> de, di, dt;
    DeviceBuffer<float> ds;
    hipError_t e;
    if ((e = stagedev::upload_pairs(de, t.et)) != hipSuccess || (e = stagedev::upload_pairs(dt, t.tt)) != hipSuccess ||
        (e = ds.replace_with(t.scan.data(), t.scan.size())) != hipSuccess ||
        (p->isc && (e = stagedev::upload_pairs(di, t.it)) != hipSuccess))
        return hip_status(e);
    const msv_status s = stagedev::adopt_tables(p, v->fn, v->waves * 64, de, di, dt);
    if (s != MSV_OK) return s;
    p->d_scan = std::move(ds);
    p->v = v;
    return MSV_OK;
}

msv_status launch(msv_fwd_profile* p, const uint8_t* d_residues, const uint64_t* d_offsets, uint64_t n,
                  const uint32_t* d_select, const uint32_t* d_select_count, float* d_scores, hipStream_t st,
                  uint32_t* errors) {
    fwdk::FwdArgs a{};
    a.etab = p->d_etab;
    a.itab = p->d_itab ? p->d_itab.get() : p->d_etab.get();
    a.ttab = p->d_ttab;
    a.scan = p->d_scan;
    a.residues = d_residues;
    a.offsets = d_offsets;
    a.select = d_select;
    a.select_count = d_select ? d_select_count : nullptr;
    a.lentab = p->d_lentab;
    a.scores = d_scores;
    a.errors = errors;
    a.n = n;
    a.lentab_n = p->lentab_n;
    a.tBM = p->tBM;
    a.tEC = p->tEC;
    a.tEJ = p->tEJ;
    // one wave per sequence
    return stagedev::run(p, st, n, static_cast<uint64_t>(p->v->waves), [&](uint32_t blocks, uint32_t* counter) {
        a.counter = counter;
        return fwdk::fwd_launch(*p->v, blocks, a, st);
    });
}

}  // namespace

extern "C" {

void msv_fwd_profile_destroy(msv_fwd_profile* p) { stagedev::close(p); }

msv_status msv_fwd_profile_reserve_length(msv_fwd_profile* p, uint64_t max_length) {
    return stagedev::reserve_length(p, max_length, [](uint32_t L, float2& t) {
        float loop, move;
        msv_sequence_transitions(L, &loop, &move);
        t.x = odds(loop);
        t.y = odds(move);
    });
}

msv_status msv_fwd_profile_create(int device, const float* match_scores, const float* insert_scores,
                                  const float* transition_scores, uint32_t model_length, float tr_B_Mk, float tr_E_C,
                                  float tr_E_J, msv_fwd_profile** out) {
    msv_status s = stagedev::check_model(match_scores, transition_scores, model_length, out);
    if (s != MSV_OK) return s;
    // one variant per S and insert mode: every one is eligible
    const fwdk::FwdVariant* v = stagedev::pick(fwdk::fwd_variants, model_length - 1, insert_scores != nullptr,
                                               [](const fwdk::FwdVariant&) { return true; });
    if (!v) return MSV_ERR_UNSUPPORTED_MODEL;
    if ((s = stagedev::check_device(device)) != MSV_OK) return s;
    return stagedev::open(device, match_scores, insert_scores, transition_scores, model_length, out,
                          [&](msv_fwd_profile* p) {
                              p->tBM = odds(tr_B_Mk);
                              p->tEC = odds(tr_E_C);
                              p->tEJ = odds(tr_E_J);
                              const msv_status si = install(p, v);
                              return si == MSV_OK
                                         ? msv_fwd_profile_reserve_length(p, stagedev::kDefaultMaxLength - 1)
                                         : si;
                          });
}

msv_status msv_fwd_profile_create_from_hmm(int device, const msv_hmm* hmm, int insert_mode, msv_fwd_profile** out) {
    return stagedev::create_from_hmm(device, hmm, insert_mode, out, msv_fwd_profile_create);
}

msv_status msv_fwd_profile_describe(const msv_fwd_profile* p, msv_fwd_info* out) {
    if (!p || !out) return MSV_ERR_INVALID_ARGUMENT;
    std::memset(out, 0, sizeof(*out));
    out->model_length = p->model_length;
    out->states_per_lane = static_cast<uint32_t>(p->v->S);
    out->match_in_lds = p->v->elds ? 1u : 0u;
    out->insert_scores = p->v->isc ? 1u : 0u;
    out->waves_per_block = static_cast<uint32_t>(p->v->waves);
    out->blocks = p->blocks;
    out->max_length = p->lentab_n ? p->lentab_n - 1 : 0;
    out->device = p->device;
    std::snprintf(out->variant, sizeof(out->variant), "%s", p->v->name);
    msvrt::kernel_footprint(p->v->fn, &out->scratch_bytes, &out->lds_bytes);
    return MSV_OK;
}

int msv_fwd_variant_count(void) { return stagedev::variant_count(fwdk::fwd_variants); }

const char* msv_fwd_variant_name(int i) { return stagedev::variant_name(fwdk::fwd_variants, i); }

msv_status msv_fwd_profile_set_variant(msv_fwd_profile* p, const char* name) {
    return stagedev::set_variant(p, fwdk::fwd_variants, name, install);
}

msv_status msv_fwd_score_batch_device(msv_fwd_profile* p, const uint8_t* d_residues, uint64_t residues_len,
                                      const uint64_t* d_offsets, uint64_t n, const uint32_t* d_select,
                                      const uint32_t* d_select_count, float* d_scores, void* stream) {
    return stagedev::score_batch_device(p, d_residues, residues_len, d_offsets, n, d_select, d_select_count, d_scores,
                                        stream, launch);
}

msv_status msv_fwd_profile_bind_stream(msv_fwd_profile* p, void* stream) { return stagedev::bind_stream(p, stream); }

msv_status msv_fwd_profile_check(msv_fwd_profile* p, void* stream) { return stagedev::check(p, stream); }

msv_status msv_fwd_score_batch(msv_fwd_profile* p, const uint8_t* residues, const uint64_t* offsets, uint64_t n,
                               float* scores, void* stream) {
    return stagedev::score_batch_host(p, residues, offsets, n, scores, stream, msv_fwd_profile_reserve_length, launch);
}

msv_status msv_fwd_pvalues_device(int device, const float* d_scores, const uint64_t* d_offsets, uint64_t n, float tau,
                                  float lambda, double* d_pvalues, void* stream) {
    if (n == 0) return MSV_OK;
    if (!d_scores || !d_offsets || !d_pvalues) return MSV_ERR_INVALID_ARGUMENT;
    DeviceGuard g(device);
    if (!g.ok) return MSV_ERR_NO_DEVICE;
    MSV_HIP(fwdk::launch_fwd_pvalues(d_scores, d_offsets, n, tau, lambda, d_pvalues, static_cast<hipStream_t>(stream)));
    return MSV_OK;
}

msv_status msv_fwd_filter_batch(msv_profile* msv, msv_vit_profile* vit, msv_fwd_profile* fwd, const uint8_t* residues,
                                const uint64_t* offsets, uint64_t n, const float* stats, double F1, double F2,
                                float* msv_scores, uint8_t* passed_msv, float* vit_scores, uint8_t* passed_vit,
                                float* fwd_scores, double* fwd_pvalues, uint64_t* n_passed_msv,
                                uint64_t* n_passed_vit) {
    return msv_fwd_filter_batch_opts(msv, vit, fwd, residues, offsets, n, stats, F1, F2, nullptr, msv_scores,
                                     passed_msv, vit_scores, passed_vit, fwd_scores, fwd_pvalues, n_passed_msv,
                                     n_passed_vit, nullptr, nullptr, nullptr);
}

msv_status msv_fwd_filter_batch_opts(msv_profile* msv, msv_vit_profile* vit, msv_fwd_profile* fwd,
                                     const uint8_t* residues, const uint64_t* offsets, uint64_t n, const float* stats,
                                     double F1, double F2, const msv_search_options* options, float* msv_scores,
                                     uint8_t* passed_msv, float* vit_scores, uint8_t* passed_vit, float* fwd_scores,
                                     double* fwd_pvalues, uint64_t* n_passed_msv, uint64_t* n_passed_vit, float* bias,
                                     uint8_t* passed_bias, uint64_t* n_passed_bias) {
    if (!msv || !vit || !fwd || !stats || !n_passed_msv || !n_passed_vit ||
        (n && (!offsets || !msv_scores || !passed_msv || !vit_scores || !passed_vit || !fwd_scores || !fwd_pvalues)))
        return MSV_ERR_INVALID_ARGUMENT;
    msv_search_options opt{};  // fields beyond the caller's struct_size read as 0
    if (options) std::memcpy(&opt, options, std::min<size_t>(sizeof(opt), options->struct_size));
    msv_bf_profile* const bf = opt.bias_filter ? opt.bias_profile : nullptr;
    if (opt.bias_filter && (!bf || !n_passed_bias || (n && (!bias || !passed_bias)) || bfdev::device_of(bf) != fwd->device))
        return MSV_ERR_INVALID_ARGUMENT;
    if (n_passed_bias) *n_passed_bias = 0;
    *n_passed_msv = *n_passed_vit = 0;
    if (n == 0) return MSV_OK;
    if (n >= (1ull << 32)) return MSV_ERR_INVALID_ARGUMENT;
    msv_kernel_info minfo{};
    msv_vit_info vinfo{};
    msv_status s = msv_profile_describe(msv, &minfo);
    if (s == MSV_OK) s = msv_vit_profile_describe(vit, &vinfo);
    if (s != MSV_OK) return s;
    if (minfo.device != fwd->device || vinfo.device != fwd->device) return MSV_ERR_INVALID_ARGUMENT;
    uint64_t longest = 0, total = 0;
    if ((s = csr_extent(offsets, n, &longest, &total)) != MSV_OK) return s;
    if (total && !residues) return MSV_ERR_INVALID_ARGUMENT;
    if (total >= msvrt::kChunkBytes) return MSV_ERR_INVALID_ARGUMENT;  // one launch per stage
    DeviceGuard g(fwd->device);
    if (!g.ok) return MSV_ERR_NO_DEVICE;
    if ((s = msv_profile_reserve_length(msv, longest)) != MSV_OK) return s;
    if ((s = msv_vit_profile_reserve_length(vit, longest)) != MSV_OK) return s;
    if ((s = msv_fwd_profile_reserve_length(fwd, longest)) != MSV_OK) return s;
    hipStream_t st = fwd->stream;
    msvrt::CsrStaging& sg = fwd->staged;
    MSV_HIP(sg.reserve_results(n, n));
    MSV_HIP(fwd->d_msv_out.reserve(n));
    MSV_HIP(fwd->d_vit_out.reserve(n));
    MSV_HIP(fwd->d_sel1.reserve(n));
    MSV_HIP(fwd->d_sel2.reserve(n));
    MSV_HIP(fwd->d_pv.reserve(n));
    uint32_t* const d_n1 = fwd->d_words + stagedev::kSelWord;
    uint32_t* const d_n2 = fwd->d_words + stagedev::kSel2Word;
    auto ninf_fill = [&](float* d) {
        return hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(d), static_cast<int>(0xff800000u), n, st);
    };
    // an early error return leaves no copy queued that reads the pinned offsets (rewritten by the next call)
    msvrt::StreamDrain drain(st);
    MSV_HIP(sg.upload(residues, offsets, 0, n, true, st, st));
    // 1. MSV over every sequence, longest first
    if ((s = msv_order_longest_first(msv, sg.d_off, n, sg.d_order, st)) != MSV_OK) return s;
    if ((s = msv_score_batch_device(msv, sg.d_res, total, sg.d_off, n, sg.d_order, fwd->d_msv_out, st)) != MSV_OK)
        return s;
    // 2. P <= F1, listed longest first; 3. Viterbi on them (-inf elsewhere)
    MSV_HIP(ninf_fill(fwd->d_vit_out));
    if ((s = msv_filter_select_device(fwd->device, fwd->d_msv_out, sg.d_off, sg.d_order, n, stats[0], stats[1], F1,
                                      nullptr, fwd->d_sel1, d_n1, st)) != MSV_OK)
        return s;
    // with the bias filter (msv.h): the bias of those (0 elsewhere: such a sequence keeps its null1 P-value and
    // stays out), then the filtered P <= F1 over every sequence in the same order gives Viterbi's list
    const uint32_t* vit_sel = fwd->d_sel1;
    const uint32_t* d_nvit = d_n1;
    float* d_bias = nullptr;
    uint32_t* d_selb = nullptr;
    uint32_t* d_nb = nullptr;
    if (bf) {
        if ((s = bfdev::cascade_buffers(bf, n, &d_bias, &d_selb, &d_nb)) != MSV_OK) return s;
        MSV_HIP(hipMemsetAsync(d_bias, 0, n * sizeof(float), st));
        if ((s = msv_bf_score_batch_device(bf, sg.d_res, total, sg.d_off, n, fwd->d_sel1, d_n1, d_bias, st)) != MSV_OK)
            return s;
        if ((s = msv_bf_filter_select_device(fwd->device, fwd->d_msv_out, d_bias, sg.d_off, sg.d_order, n, stats[0],
                                             stats[1], F1, nullptr, d_selb, d_nb, st)) != MSV_OK)
            return s;
        vit_sel = d_selb;
        d_nvit = d_nb;
    }
    if ((s = msv_vit_score_batch_device(vit, sg.d_res, total, sg.d_off, n, vit_sel, d_nvit, fwd->d_vit_out, st)) !=
        MSV_OK)
        return s;
    // 4. P <= F2 over the Viterbi scores (a sequence that did not run has -inf, so P = 1); 5. Forward on them
    MSV_HIP(ninf_fill(sg.d_scores));
    s = bf ? msv_bf_filter_select_device(fwd->device, fwd->d_vit_out, d_bias, sg.d_off, sg.d_order, n, stats[2],
                                         stats[3], F2, nullptr, fwd->d_sel2, d_n2, st)
           : msv_filter_select_device(fwd->device, fwd->d_vit_out, sg.d_off, sg.d_order, n, stats[2], stats[3], F2,
                                      nullptr, fwd->d_sel2, d_n2, st);
    if (s != MSV_OK) return s;
    if ((s = launch(fwd, sg.d_res, sg.d_off, n, fwd->d_sel2, d_n2, sg.d_scores, st, fwd->d_words + kHostErrWord)) !=
        MSV_OK)
        return s;
    // 6. Forward P-values (a sequence that did not run has -inf: bits < tau, P = 1)
    // (with the bias filter they are taken on the host from the downloaded scores and bias, below: the outputs are
    // host arrays, and fwd_pvalues is then msv_bf_pvalues on fwd_scores and bias to the last bit)
    if (!bf) MSV_HIP(fwdk::launch_fwd_pvalues(sg.d_scores, sg.d_off, n, stats[4], stats[5], fwd->d_pv, st));
    uint32_t counts[2] = {0, 0};
    uint32_t count_b = 0;
    if (bf) {
        MSV_HIP(hipMemcpyAsync(bias, d_bias, n * sizeof(float), hipMemcpyDeviceToHost, st));
        MSV_HIP(hipMemcpyAsync(&count_b, d_nb, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    }
    MSV_HIP(hipMemcpyAsync(msv_scores, fwd->d_msv_out, n * sizeof(float), hipMemcpyDeviceToHost, st));
    MSV_HIP(hipMemcpyAsync(vit_scores, fwd->d_vit_out, n * sizeof(float), hipMemcpyDeviceToHost, st));
    MSV_HIP(hipMemcpyAsync(fwd_scores, sg.d_scores, n * sizeof(float), hipMemcpyDeviceToHost, st));
    if (!bf) MSV_HIP(hipMemcpyAsync(fwd_pvalues, fwd->d_pv, n * sizeof(double), hipMemcpyDeviceToHost, st));
    MSV_HIP(hipMemcpyAsync(counts, d_n1, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    MSV_HIP(hipStreamSynchronize(st));
    drain.disarm();
    if ((s = stagedev::survivor_mask(st, counts[0], fwd->d_sel1, passed_msv, n)) != MSV_OK) return s;
    if ((s = stagedev::survivor_mask(st, counts[1], fwd->d_sel2, passed_vit, n)) != MSV_OK) return s;
    *n_passed_msv = counts[0];
    *n_passed_vit = counts[1];
    if (bf) {
        if ((s = msv_bf_pvalues(fwd_scores, bias, offsets, n, stats[4], stats[5], MSV_BF_EXPONENTIAL, fwd_pvalues)) !=
            MSV_OK)
            return s;
        if ((s = stagedev::survivor_mask(st, count_b, d_selb, passed_bias, n)) != MSV_OK) return s;
        *n_passed_bias = count_b;
    } else {
        if (bias) std::fill(bias, bias + n, 0.0f);
        if (passed_bias) std::copy(passed_msv, passed_msv + n, passed_bias);
        if (n_passed_bias) *n_passed_bias = counts[0];
    }
    // every stage's word is read, so each call clears its own bits (a bad residue latches all three)
    s = msv_profile_check(msv, st);
    const msv_status vs = msv_vit_profile_check(vit, st);
    const msv_status fs = stagedev::read_errors(fwd, kHostErrWord, st);
    const msv_status bs = bf ? msv_bf_profile_check(bf, st) : MSV_OK;
    return s != MSV_OK ? s : vs != MSV_OK ? vs : fs != MSV_OK ? fs : bs;
}

}  // extern "C"
