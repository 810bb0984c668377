// vit_device.cpp -- C-ABI of the Viterbi stage (msv.h) on the HIP runtime.
//
// The reference parses insert emissions, transitions and STATS LOCAL VITERBI (Profile_HMM.cpp:86-87,
// 107-120) and never scores with them.  A msv_vit_profile holds the kernel-layout tables of one compiled
// variant (vit_kernel.hip), its own per-length {tr_loop, tr_move} table (host logf, MSV_HMM.cpp:59-64)
// and self-resetting dequeue counters (one pair per launch slot, launch_ring.h, so one profile may be
// driven from several streams at once); a batch -- typically the MSV filter's survivors, selected on the
// device -- is one persistent launch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <new>
#include <vector>

#include "hip_rt.h"
#include "host_cpu.h"
#include "launch_ring.h"
#include "msv.h"
#include "msv_kernel.h"
#include "vit_kernel.h"
#include "vit_profile.h"

using msvrt::csr_extent;
using msvrt::DeviceBuffer;
using msvrt::DeviceGuard;
using msvrt::hip_status;

// table_layout.cpp builds the tables without vit_kernel.h
static_assert(vitk::kRows == 20 && vitk::kTransitions == 7 && vitk::kLanes == 64, "table_layout.cpp's shape");
static_assert(vitk::MM_IN == 0 && vitk::IM_IN == 1 && vitk::DM_IN == 2 && vitk::MI == 3 && vitk::II == 4 &&
                  vitk::MD_IN == 5 && vitk::DD_IN == 6,
              "table_layout.cpp's slot arrays");

using vitdev::kErrWord;
using vitdev::kHostErrWord;
using vitdev::kSelWord;
using vitdev::kWords;
using vitdev::read_errors;

namespace vitdev {

msv_status err_status(uint32_t err) {
    if (err & msvk::kErrBadResidue) return MSV_ERR_BAD_RESIDUE;
    if (err & msvk::kErrTooLong) return MSV_ERR_SEQUENCE_TOO_LONG;
    if (err & msvk::kErrBadOrder) return MSV_ERR_INVALID_ARGUMENT;  // a survivors entry outside the batch
    if (err & msvk::kErrTeamHang) return MSV_ERR_HIP;
    return err ? MSV_ERR_INVALID_ARGUMENT : MSV_OK;
}

}  // namespace vitdev

namespace {

constexpr uint32_t kDefaultMaxLength = 131072;
// The automatic choice covering `states`: among the variants marked `pick` (one per S and insert mode, by
// measurement), the fewest slots.  Informative insert scores need an isc variant.
const vitk::VitVariant* pick_variant(uint32_t states, bool isc) {
    int n = 0;
    const vitk::VitVariant* all = vitk::vit_variants(&n);
    const vitk::VitVariant* best = nullptr;
    for (int i = 0; i < n; ++i) {
        const vitk::VitVariant& v = all[i];
        if (!v.pick || v.isc != isc || static_cast<uint32_t>(v.states()) < states) continue;
        if (!best || v.states() < best->states()) best = &v;
    }
    return best;
}

// Lays the variant's tables out (msv_host::vit_tables) and uploads them, all three or none: each goes into a
// fresh buffer, and the profile adopts them together.
msv_status install(msv_vit_profile* p, const vitk::VitVariant* v) {
    const msv_host::VitTables t = msv_host::vit_tables(p->msc.data(), p->isc_tab.data(), p->tsc.data(), p->model_length,
                                                       v->S, v->team, p->isc);
    auto upload = [](DeviceBuffer<float2>& d, const std::vector<float>& pairs) {
        return d.replace_with(reinterpret_cast<const float2*>(pairs.data()), pairs.size() / 2);
    };
    DeviceBuffer<float2> de, di, dt;
    hipError_t e;
    if ((e = upload(de, t.et)) != hipSuccess || (e = upload(dt, t.tt)) != hipSuccess ||
        (p->isc && (e = upload(di, t.it)) != hipSuccess))
        return hip_status(e);
    int blocks = 0;
    if ((e = msvrt::resident_blocks(p->device, v->fn, v->waves * 64, &blocks)) != hipSuccess) return hip_status(e);
    // the previous tables may still be read by a launch in flight on any stream
    if (p->d_etab || p->d_ttab) (void)hipDeviceSynchronize();
    p->d_etab = std::move(de);
    p->d_itab = std::move(di);
    p->d_ttab = std::move(dt);
    p->v = v;
    p->blocks = static_cast<uint32_t>(std::max(1, blocks));
    return MSV_OK;
}

hipStream_t stream_of(const msv_vit_profile* p, void* stream) {
    return stream ? static_cast<hipStream_t>(stream) : static_cast<hipStream_t>(p->stream);
}

// Every launch takes the next counter slot (a slot whose previous launch ran on another stream is reused
// only after it: launch_ring.h), so launches of one profile on several streams never share a counter.
// `errors` is the word the kernel latches its error bits into (device launches: kErrWord; host calls:
// kHostErrWord).
msv_status launch(msv_vit_profile* p, const uint8_t* d_residues, const uint64_t* d_offsets, uint64_t n,
                  const uint32_t* d_select, const uint32_t* d_select_count, float* d_scores, hipStream_t st,
                  uint32_t* errors, hipEvent_t start = nullptr, hipEvent_t stop = nullptr) {
    if (n == 0) return MSV_OK;
    if (n >= (1ull << 32)) return MSV_ERR_INVALID_ARGUMENT;
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
    // one wave (team) per sequence: no more workgroups than the items need (a device count is bounded by n)
    const uint64_t per_block = static_cast<uint64_t>(p->v->sequences_per_block());
    const uint64_t need = (n + per_block - 1) / per_block;
    const uint32_t blocks = static_cast<uint32_t>(std::min<uint64_t>(p->blocks, need));
    if (!start && !stop && (p->time_start || p->time_stop)) {
        start = p->time_start;
        stop = p->time_stop;
        p->time_start = p->time_stop = nullptr;
    }
    // a slot's counters are put back to zero by the last wave of every launch; a failed launch may leave
    // them dirty, so the slot's next launch resets them explicitly (LaunchRing::run)
    const bool lazy = st == p->stream || (p->bound && st == p->bound);
    MSV_HIP(p->kernels.run(st, lazy, p->d_words.get(), 2, [&](uint32_t* counter) {
        a.counter = counter;
        return vitk::vit_launch(*p->v, blocks, a, st, start, stop);
    }));
    return MSV_OK;
}

}  // namespace

namespace vitdev {

// Reads (and clears when set) one error word of the profile on `st`, synchronously.
msv_status read_errors(msv_vit_profile* p, int word, hipStream_t st) {
    uint32_t err = 0;
    MSV_HIP(hipMemcpyAsync(&err, p->d_words + word, sizeof(err), hipMemcpyDeviceToHost, st));
    MSV_HIP(hipStreamSynchronize(st));
    if (err) {
        MSV_HIP(hipMemsetAsync(p->d_words + word, 0, sizeof(uint32_t), st));
        MSV_HIP(hipStreamSynchronize(st));
    }
    return err_status(err);
}

}  // namespace vitdev

extern "C" {

void msv_vit_profile_destroy(msv_vit_profile* p) {
    if (!p) return;
    DeviceGuard g(p->device);
    (void)hipDeviceSynchronize();
    delete p;
}

msv_status msv_vit_profile_reserve_length(msv_vit_profile* p, uint64_t max_length) {
    if (!p) return MSV_ERR_INVALID_ARGUMENT;
    if (max_length >= (1ull << 31)) return MSV_ERR_SEQUENCE_TOO_LONG;
    const uint32_t need = static_cast<uint32_t>(max_length) + 1;
    if (need <= p->lentab_n) return MSV_OK;
    DeviceGuard g(p->device);
    if (!g.ok) return MSV_ERR_NO_DEVICE;
    const uint32_t n = std::max(need, p->lentab_n * 2);
    std::vector<float2> host(n);
    for (uint32_t L = 0; L < n; ++L) msv_sequence_transitions(L, &host[L].x, &host[L].y);  // MSV_HMM.cpp:59-64
    MSV_HIP(p->d_lentab.replace_with(host.data(), n));
    p->lentab_n = n;
    return MSV_OK;
}

msv_status msv_vit_profile_create(int device, const float* match_scores, const float* insert_scores,
                                  const float* transition_scores, uint32_t model_length, float tr_B_Mk, float tr_E_C,
                                  float tr_E_J, msv_vit_profile** out) {
    if (!match_scores || !transition_scores || !out || model_length < 2) return MSV_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    // The kernel leaves D(LENG) out of E, exact only while every transition it reads (nodes 1 .. LENG-1,
    // install) is <= 0 (then every D is bounded by an M of its row); log-probabilities always are.
    for (size_t k = 1; k + 1 < model_length; ++k)
        for (int t = 0; t < 7; ++t)
            if (!(transition_scores[k * 7 + t] <= 0.0f)) return MSV_ERR_INVALID_ARGUMENT;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return MSV_ERR_NO_DEVICE;
    if (device < 0 || device >= ndev) return MSV_ERR_NO_DEVICE;
    const vitk::VitVariant* v = pick_variant(model_length - 1, insert_scores != nullptr);
    if (!v) return MSV_ERR_UNSUPPORTED_MODEL;
    DeviceGuard g(device);
    if (!g.ok) return MSV_ERR_NO_DEVICE;
    auto* p = new (std::nothrow) msv_vit_profile;
    if (!p) return MSV_ERR_OUT_OF_MEMORY;
    p->device = device;
    p->model_length = model_length;
    p->isc = insert_scores != nullptr;
    p->tr_B_Mk = tr_B_Mk;
    p->tr_E_C = tr_E_C;
    p->tr_E_J = tr_E_J;
    const size_t M = model_length;
    p->msc.assign(match_scores, match_scores + 20 * M);
    if (insert_scores) p->isc_tab.assign(insert_scores, insert_scores + 20 * M);
    p->tsc.assign(transition_scores, transition_scores + 7 * M);
    hipError_t e;
    if ((e = p->stream.create(hipStreamNonBlocking)) != hipSuccess ||
        (e = p->kernels.create_events()) != hipSuccess || (e = p->d_words.reserve(kWords)) != hipSuccess ||
        (e = hipMemset(p->d_words, 0, kWords * sizeof(uint32_t))) != hipSuccess) {
        msv_vit_profile_destroy(p);
        return hip_status(e);
    }
    msv_status s = install(p, v);
    if (s == MSV_OK) s = msv_vit_profile_reserve_length(p, kDefaultMaxLength - 1);
    if (s != MSV_OK) {
        msv_vit_profile_destroy(p);
        return s;
    }
    *out = p;
    return MSV_OK;
}

msv_status msv_vit_profile_create_from_hmm(int device, const msv_hmm* hmm, int insert_mode, msv_vit_profile** out) {
    if (!hmm || !out) return MSV_ERR_INVALID_ARGUMENT;
    const size_t M = msv_hmm_model_length(hmm);
    std::vector<float> msc(20 * M), isc(20 * M), tsc(7 * M);
    float b, c, j;
    msv_status s = msv_hmm_viterbi_scores(hmm, insert_mode, msc.data(), isc.data(), tsc.data(), &b, &c, &j);
    if (s != MSV_OK) return s;
    return msv_vit_profile_create(device, msc.data(), insert_mode == MSV_INSERTS_LOG_ODDS ? isc.data() : nullptr,
                                  tsc.data(), static_cast<uint32_t>(M), b, c, j, out);
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
    hipFuncAttributes fa{};
    if (hipFuncGetAttributes(&fa, p->v->fn) == hipSuccess) {
        out->scratch_bytes = static_cast<uint32_t>(fa.localSizeBytes);
        out->lds_bytes = static_cast<uint32_t>(fa.sharedSizeBytes);  // the kernel's own static LDS, exactly
    }
    return MSV_OK;
}

int msv_vit_variant_count(void) {
    int n = 0;
    vitk::vit_variants(&n);
    return n;
}

const char* msv_vit_variant_name(int i) {
    int n = 0;
    const vitk::VitVariant* all = vitk::vit_variants(&n);
    return (i >= 0 && i < n) ? all[i].name : "";
}

msv_status msv_vit_profile_set_variant(msv_vit_profile* p, const char* name) {
    if (!p || !name) return MSV_ERR_INVALID_ARGUMENT;
    int n = 0;
    const vitk::VitVariant* all = vitk::vit_variants(&n);
    for (int i = 0; i < n; ++i)
        if (std::strcmp(all[i].name, name) == 0) {
            if (all[i].isc != p->isc || static_cast<uint32_t>(all[i].states()) < p->model_length - 1)
                return MSV_ERR_UNSUPPORTED_MODEL;
            DeviceGuard g(p->device);
            if (!g.ok) return MSV_ERR_NO_DEVICE;
            return install(p, &all[i]);
        }
    return MSV_ERR_INVALID_ARGUMENT;
}

msv_status msv_vit_score_batch_device(msv_vit_profile* p, const uint8_t* d_residues, uint64_t residues_len,
                                      const uint64_t* d_offsets, uint64_t n, const uint32_t* d_select,
                                      const uint32_t* d_select_count, float* d_scores, void* stream) {
    if (!p || (n && (!d_offsets || !d_scores))) return MSV_ERR_INVALID_ARGUMENT;
    if (n && residues_len && !d_residues) return MSV_ERR_INVALID_ARGUMENT;
    if (d_select_count && !d_select) return MSV_ERR_INVALID_ARGUMENT;
    DeviceGuard g(p->device);
    if (!g.ok) return MSV_ERR_NO_DEVICE;
    return launch(p, d_residues, d_offsets, n, d_select, d_select_count, d_scores, stream_of(p, stream),
                  p->d_words + kErrWord);
}

msv_status msv_vit_profile_bind_stream(msv_vit_profile* p, void* stream) {
    if (!p) return MSV_ERR_INVALID_ARGUMENT;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (st == p->bound) return MSV_OK;
    DeviceGuard g(p->device);
    if (!g.ok) return MSV_ERR_NO_DEVICE;
    if (p->bound) MSV_HIP(p->kernels.flush(p->bound));  // the old stream loses its guarantee
    p->bound = st;
    return MSV_OK;
}

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

msv_status msv_vit_profile_check(msv_vit_profile* p, void* stream) {
    if (!p) return MSV_ERR_INVALID_ARGUMENT;
    DeviceGuard g(p->device);
    if (!g.ok) return MSV_ERR_NO_DEVICE;
    return read_errors(p, kErrWord, stream_of(p, stream));
}

msv_status msv_vit_score_batch(msv_vit_profile* p, const uint8_t* residues, const uint64_t* offsets, uint64_t n,
                               float* scores, void* stream) {
    if (!p || (n && (!offsets || !scores))) return MSV_ERR_INVALID_ARGUMENT;
    if (n == 0) return MSV_OK;
    uint64_t longest = 0, total = 0;
    msv_status s = csr_extent(offsets, n, &longest, &total);
    if (s != MSV_OK) return s;
    if (total && !residues) return MSV_ERR_INVALID_ARGUMENT;
    DeviceGuard g(p->device);
    if (!g.ok) return MSV_ERR_NO_DEVICE;
    s = msv_vit_profile_reserve_length(p, longest);
    if (s != MSV_OK) return s;
    hipStream_t st = stream_of(p, stream);
    msvrt::CsrStaging& sg = p->staged;
    MSV_HIP(sg.d_scores.reserve(n));
    // an early error return leaves no copy queued that reads the pinned offsets (rewritten by the next call)
    msvrt::StreamDrain drain(st);
    MSV_HIP(sg.upload(residues, offsets, 0, n, true, st, st));
    s = launch(p, sg.d_res, sg.d_off, n, nullptr, nullptr, sg.d_scores, st, p->d_words + kHostErrWord);
    if (s != MSV_OK) return s;
    MSV_HIP(hipMemcpyAsync(scores, sg.d_scores, n * sizeof(float), hipMemcpyDeviceToHost, st));
    drain.disarm();
    return read_errors(p, kHostErrWord, st);  // synchronises
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
    std::vector<uint32_t> sel;
    MSV_HIP(hipStreamSynchronize(st));
    drain.disarm();
    if (count) {
        sel.resize(count);
        MSV_HIP(hipMemcpyAsync(sel.data(), vit->d_sel, count * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        MSV_HIP(hipStreamSynchronize(st));
    }
    std::fill(passed, passed + n, static_cast<uint8_t>(0));
    for (uint32_t x : sel) passed[x] = 1;
    *n_passed = count;
    // both stages' words are read, so each call clears its own bits (a bad residue in a survivor latches both)
    s = msv_profile_check(msv, st);
    const msv_status vs = read_errors(vit, kHostErrWord, st);
    return s != MSV_OK ? s : vs;
}

}  // extern "C"
