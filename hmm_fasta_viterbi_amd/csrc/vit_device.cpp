// vit_device.cpp -- C-ABI of the Viterbi stage (msv.h) on the HIP runtime.
//
// The reference parses insert emissions, transitions and STATS LOCAL VITERBI (Profile_HMM.cpp:86-87,
// 107-120) and never scores with them.  A msv_vit_profile is a stage profile (stage_profile.h: tables, length
// table, launch slots, streams, error words) of one compiled variant of vit_kernel.hip / vit_team.hip, with
// log-score tables and a host-logf {tr_loop, tr_move} table (MSV_HMM.cpp:59-64); a batch -- typically the MSV
// filter's survivors, selected on the device -- is one persistent launch.  The entry points are their argument
// checks and one call into stage_profile.h; what is only the Viterbi stage's stands here.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <vector>

#include "hip_rt.h"
#include "host_cpu.h"
#include "msv.h"
#include "msv_kernel.h"
#include "vit_kernel.h"
#include "vit_profile.h"

using msvrt::csr_extent;
using msvrt::DeviceBuffer;
using msvrt::DeviceGuard;
using msvrt::hip_status;
using stagedev::kHostErrWord;
using stagedev::kSelWord;

// table_layout.cpp builds the tables without vit_kernel.h
static_assert(vitk::kRows == 20 && vitk::kTransitions == 7 && vitk::kLanes == 64, "table_layout.cpp's shape");
static_assert(vitk::MM_IN == 0 && vitk::IM_IN == 1 && vitk::DM_IN == 2 && vitk::MI == 3 && vitk::II == 4 &&
                  vitk::MD_IN == 5 && vitk::DD_IN == 6,
              "table_layout.cpp's slot arrays");

namespace {

// Lays the variant's tables out (msv_host::vit_tables) and uploads them, all three or none: each goes into a
// fresh buffer, and the profile adopts them together.
msv_status install(msv_vit_profile* p, const vitk::VitVariant* v) {
    const msv_host::VitTables t = msv_host::vit_tables(p->msc.data(), p->isc_tab.data(), p->tsc.data(), p->model_length,
                                                       v->S, v->team, p->isc);
    DeviceBuffer<float2> de, di, dt;
    hipError_t e;
    if ((e = stagedev::upload_pairs(de, t.et)) != hipSuccess || (e = stagedev::upload_pairs(dt, t.tt)) != hipSuccess ||
        (p->isc && (e = stagedev::upload_pairs(di, t.it)) != hipSuccess))
        return hip_status(e);
    const msv_status s = stagedev::adopt_tables(p, v->fn, v->waves * 64, de, di, dt);
    if (s == MSV_OK) p->v = v;
    return s;
}

msv_status launch(msv_vit_profile* p, const uint8_t* d_residues, const uint64_t* d_offsets, uint64_t n,
                  const uint32_t* d_select, const uint32_t* d_select_count, float* d_scores, hipStream_t st,
                  uint32_t* errors) {
    vitk::VitArgs a{};
    a.etab = p->d_etab;
    a.itab = p->d_itab ? p->d_itab.get() : p->d_etab.get();
    a.ttab = p->d_ttab;
    a.residues = d_residues;
    a.offsets = d_offsets;
    a.select = d_select;
    a.select_count = d_select ? d_select_count : nullptr;
    a.lentab = p->d_lentab;
    a.scores = d_scores;
    a.errors = errors;
    a.n = n;
    a.lentab_n = p->lentab_n;
    a.tr_B_Mk = p->tr_B_Mk;
    a.tr_E_C = p->tr_E_C;
    a.tr_E_J = p->tr_E_J;
    a.stamps = p->d_stamps;
    // one wave (team) per sequence
    return stagedev::run(p, st, n, static_cast<uint64_t>(p->v->sequences_per_block()),
                         [&](uint32_t blocks, uint32_t* counter) {
                             a.counter = counter;
                             const hipEvent_t start = p->time_start, stop = p->time_stop;  // this launch's only
                             p->time_start = p->time_stop = nullptr;
                             return vitk::vit_launch(*p->v, blocks, a, st, start, stop);
                         });
}

}  // namespace

extern "C" {

void msv_vit_profile_destroy(msv_vit_profile* p) { stagedev::close(p); }

msv_status msv_vit_profile_reserve_length(msv_vit_profile* p, uint64_t max_length) {
    return stagedev::reserve_length(p, max_length, [](uint32_t L, float2& t) {
        msv_sequence_transitions(L, &t.x, &t.y);  // MSV_HMM.cpp:59-64
    });
}

msv_status msv_vit_profile_create(int device, const float* match_scores, const float* insert_scores,
                                  const float* transition_scores, uint32_t model_length, float tr_B_Mk, float tr_E_C,
                                  float tr_E_J, msv_vit_profile** out) {
    msv_status s = stagedev::check_model(match_scores, transition_scores, model_length, out);
    if (s == MSV_OK) s = stagedev::check_device(device);
    if (s != MSV_OK) return s;
    // among the variants marked `pick` (one per S and insert mode, by measurement)
    const vitk::VitVariant* v = stagedev::pick(vitk::vit_variants, model_length - 1, insert_scores != nullptr,
                                               [](const vitk::VitVariant& x) { return x.pick; });
    if (!v) return MSV_ERR_UNSUPPORTED_MODEL;
    return stagedev::open(device, match_scores, insert_scores, transition_scores, model_length, out,
                          [&](msv_vit_profile* p) {
                              p->tr_B_Mk = tr_B_Mk;
                              p->tr_E_C = tr_E_C;
                              p->tr_E_J = tr_E_J;
                              const msv_status si = install(p, v);
                              return si == MSV_OK
                                         ? msv_vit_profile_reserve_length(p, stagedev::kDefaultMaxLength - 1)
                                         : si;
                          });
}

msv_status msv_vit_profile_create_from_hmm(int device, const msv_hmm* hmm, int insert_mode, msv_vit_profile** out) {
    return stagedev::create_from_hmm(device, hmm, insert_mode, out, msv_vit_profile_create);
}

msv_status msv_vit_profile_describe(const msv_vit_profile* p, msv_vit_info* out) {
    if (!p || !out) return MSV_ERR_INVALID_ARGUMENT;
    std::memset(out, 0, sizeof(*out));
    out->model_length = p->model_length;
    out->states_per_lane = static_cast<uint32_t>(p->v->S);
    out->transitions_in_registers = static_cast<uint32_t>(p->v->ntreg);
    out->match_in_lds = p->v->elds ? 1u : 0u;
    out->insert_scores = p->v->isc ? 1u : 0u;
    out->waves_per_block = static_cast<uint32_t>(p->v->waves);
    out->waves_per_sequence = static_cast<uint32_t>(p->v->team);
    out->blocks = p->blocks;
    out->lds_bytes = static_cast<uint32_t>(p->v->lds_bytes);
    out->max_length = p->lentab_n ? p->lentab_n - 1 : 0;
    out->device = p->device;
    std::snprintf(out->variant, sizeof(out->variant), "%s", p->v->name);
    msvrt::kernel_footprint(p->v->fn, &out->scratch_bytes, &out->lds_bytes);  // (the kernel's own static LDS)
    return MSV_OK;
}

int msv_vit_variant_count(void) { return stagedev::variant_count(vitk::vit_variants); }

const char* msv_vit_variant_name(int i) { return stagedev::variant_name(vitk::vit_variants, i); }

msv_status msv_vit_profile_set_variant(msv_vit_profile* p, const char* name) {
    return stagedev::set_variant(p, vitk::vit_variants, name, install);
}

msv_status msv_vit_score_batch_device(msv_vit_profile* p, const uint8_t* d_residues, uint64_t residues_len,
                                      const uint64_t* d_offsets, uint64_t n, const uint32_t* d_select,
                                      const uint32_t* d_select_count, float* d_scores, void* stream) {
    return stagedev::score_batch_device(p, d_residues, residues_len, d_offsets, n, d_select, d_select_count, d_scores,
                                        stream, launch);
}

msv_status msv_vit_profile_bind_stream(msv_vit_profile* p, void* stream) { return stagedev::bind_stream(p, stream); }

// Diagnostic (bench.py): the next launch updates these two HIP events with its own start and end
// (hipExtLaunchKernel), so a timed launch adds no marker packets to its stream.  Not in msv.h.
msv_status msv_vit_debug_time_next_launch(msv_vit_profile* p, void* start, void* stop) {
    if (!p) return MSV_ERR_INVALID_ARGUMENT;
    p->time_start = static_cast<hipEvent_t>(start);
    p->time_stop = static_cast<hipEvent_t>(stop);
    return MSV_OK;
}

// Diagnostic (tools/vit_timeline.py, not in msv.h): subsequent team-kernel launches write their timeline to
// d_stamps (4 uint64 per list entry, then 4 per wave; the caller sizes it), nullptr turns it off.
msv_status msv_vit_debug_set_stamps(msv_vit_profile* p, uint64_t* d_stamps) {
    if (!p) return MSV_ERR_INVALID_ARGUMENT;
    p->d_stamps = d_stamps;
    return MSV_OK;
}

msv_status msv_vit_profile_check(msv_vit_profile* p, void* stream) { return stagedev::check(p, stream); }

msv_status msv_vit_score_batch(msv_vit_profile* p, const uint8_t* residues, const uint64_t* offsets, uint64_t n,
                               float* scores, void* stream) {
    return stagedev::score_batch_host(p, residues, offsets, n, scores, stream, msv_vit_profile_reserve_length, launch);
}

msv_status msv_filter_select_device(int device, const float* d_scores, const uint64_t* d_offsets,
                                    const uint32_t* d_order, uint64_t n, float mu, float lambda, double threshold,
                                    double* d_pvalues, uint32_t* d_selected, uint32_t* d_count, void* stream) {
    if (!d_count || (n && (!d_scores || !d_offsets || !d_selected))) return MSV_ERR_INVALID_ARGUMENT;
    if (n >= (1ull << 32)) return MSV_ERR_INVALID_ARGUMENT;
    // No default stream here: NULL would be the legacy null stream, unordered with the profiles' own
    // non-blocking streams that msv_score_batch_device / msv_vit_score_batch_device take for NULL.
    if (!stream) return MSV_ERR_INVALID_ARGUMENT;
    DeviceGuard g(device);
    if (!g.ok) return MSV_ERR_NO_DEVICE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    return hip_status(
        vitk::launch_select(d_scores, d_offsets, d_order, n, mu, lambda, threshold, d_pvalues, d_selected, d_count, st));
}

msv_status msv_vit_filter_batch(msv_profile* msv, msv_vit_profile* vit, const uint8_t* residues,
                                const uint64_t* offsets, uint64_t n, float msv_mu, float msv_lambda, double F1,
                                float* msv_scores, uint8_t* passed, float* vit_scores, uint64_t* n_passed) {
    if (!msv || !vit || (n && (!offsets || !msv_scores || !passed || !vit_scores)) || !n_passed)
        return MSV_ERR_INVALID_ARGUMENT;
    *n_passed = 0;
    if (n == 0) return MSV_OK;
    if (n >= (1ull << 32)) return MSV_ERR_INVALID_ARGUMENT;
    msv_kernel_info info{};
    msv_status s = msv_profile_describe(msv, &info);
    if (s != MSV_OK) return s;
    if (info.device != vit->device) return MSV_ERR_INVALID_ARGUMENT;
    uint64_t longest = 0, total = 0;
    if ((s = csr_extent(offsets, n, &longest, &total)) != MSV_OK) return s;
    if (total && !residues) return MSV_ERR_INVALID_ARGUMENT;
    if (total >= msvrt::kChunkBytes) return MSV_ERR_INVALID_ARGUMENT;  // one launch per stage
    DeviceGuard g(vit->device);
    if (!g.ok) return MSV_ERR_NO_DEVICE;
    if ((s = msv_profile_reserve_length(msv, longest)) != MSV_OK) return s;
    if ((s = msv_vit_profile_reserve_length(vit, longest)) != MSV_OK) return s;
    hipStream_t st = vit->stream;
    msvrt::CsrStaging& sg = vit->staged;
    MSV_HIP(sg.reserve_results(n, n));
    MSV_HIP(vit->d_msc_out.reserve(n));
    MSV_HIP(vit->d_sel.reserve(n));
    // an early error return leaves no copy queued that reads the pinned offsets (rewritten by the next call)
    msvrt::StreamDrain drain(st);
    MSV_HIP(sg.upload(residues, offsets, 0, n, true, st, st));
    // MSV over every sequence, longest first
    if ((s = msv_order_longest_first(msv, sg.d_off, n, sg.d_order, st)) != MSV_OK) return s;
    if ((s = msv_score_batch_device(msv, sg.d_res, total, sg.d_off, n, sg.d_order, vit->d_msc_out, st)) != MSV_OK)
        return s;
    // survivors (P <= F1) -> Viterbi, all on the device; non-survivors keep -inf (0xff800000)
    MSV_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(sg.d_scores.get()), static_cast<int>(0xff800000u), n, st));
    // survivors listed longest first (the MSV launch's order): the Viterbi launch's tail is its shortest ones
    if ((s = msv_filter_select_device(vit->device, vit->d_msc_out, sg.d_off, sg.d_order, n, msv_mu, msv_lambda, F1,
                                      nullptr, vit->d_sel, vit->d_words + kSelWord, st)) != MSV_OK)
        return s;
    if ((s = launch(vit, sg.d_res, sg.d_off, n, vit->d_sel, vit->d_words + kSelWord, sg.d_scores, st,
                    vit->d_words + kHostErrWord)) != MSV_OK)
        return s;
    uint32_t count = 0;
    MSV_HIP(hipMemcpyAsync(msv_scores, vit->d_msc_out, n * sizeof(float), hipMemcpyDeviceToHost, st));
    MSV_HIP(hipMemcpyAsync(vit_scores, sg.d_scores, n * sizeof(float), hipMemcpyDeviceToHost, st));
    MSV_HIP(hipMemcpyAsync(&count, vit->d_words + kSelWord, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    MSV_HIP(hipStreamSynchronize(st));
    drain.disarm();
    if ((s = stagedev::survivor_mask(st, count, vit->d_sel, passed, n)) != MSV_OK) return s;
    *n_passed = count;
    // both stages' words are read, so each call clears its own bits (a bad residue in a survivor latches both)
    s = msv_profile_check(msv, st);
    const msv_status vs = stagedev::read_errors(vit, kHostErrWord, st);
    return s != MSV_OK ? s : vs;
}

}  // extern "C"
