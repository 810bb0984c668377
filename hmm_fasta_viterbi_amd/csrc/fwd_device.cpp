// fwd_device.cpp -- C-ABI of the Forward stage (msv.h) on the HIP runtime.
//
// A msv_fwd_profile holds the kernel-layout odds tables of one compiled variant (fwd_kernel.hip) with the D-scan
// constants, its own per-length odds {loop, move} table and self-resetting dequeue counters (one pair per launch
// slot, launch_ring.h, so one profile may be driven from several streams at once), exactly as msv_vit_profile
// does; a batch -- typically the Viterbi filter's survivors, selected on the device -- is one persistent launch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>
#include <vector>

#include "fwd_host.h"
#include "fwd_kernel.h"
#include "hip_rt.h"
#include "launch_ring.h"
#include "msv.h"
#include "msv_kernel.h"

using msvrt::csr_extent;
using msvrt::DeviceBuffer;
using msvrt::DeviceGuard;
using msvrt::hip_status;

namespace {

// d_words: [2k, 2k+1] = launch slot k's dequeue counters (zero between launches), [kErrWord] = sticky error bits
// of device launches (msv_fwd_profile_check), [kHostErrWord] = the error bits of the synchronous host calls,
// [kSel1Word], [kSel2Word] = msv_fwd_filter_batch's survivor counts.
constexpr int kLaunchSlots = 8;
constexpr int kErrWord = 2 * kLaunchSlots;
constexpr int kHostErrWord = kErrWord + 1;
constexpr int kSel1Word = kHostErrWord + 1;
constexpr int kSel2Word = kSel1Word + 1;
constexpr int kWords = kSel2Word + 1;
constexpr uint32_t kDefaultMaxLength = 131072;

}  // namespace

struct msv_fwd_profile {
    int device = 0;
    uint32_t model_length = 0;  // LENG + 1
    bool isc = false;
    float tBM = 0, tEC = 0, tEJ = 0;       // odds of tr_B_Mk, tr_E_C, tr_E_J
    std::vector<float> msc, isc_tab, tsc;  // host copies of the score tables (re-laid when the variant changes)
    const fwdk::FwdVariant* v = nullptr;
    uint32_t blocks = 0;  // persistent grid of a full launch
    DeviceBuffer<float2> d_etab, d_itab, d_ttab;
    DeviceBuffer<float> d_scan;
    DeviceBuffer<float2> d_lentab;
    uint32_t lentab_n = 0;
    DeviceBuffer<uint32_t> d_words;
    msvrt::LaunchRing<kLaunchSlots> kernels;
    msvrt::Stream stream;
    hipStream_t bound = nullptr;
    // msv_fwd_score_batch / msv_fwd_filter_batch staging (staged.d_scores: the Forward scores); the cascade's
    // MSV and Viterbi scores, its two survivor lists and the P-values beside it
    msvrt::CsrStaging staged;
    DeviceBuffer<float> d_msv_out, d_vit_out;
    DeviceBuffer<uint32_t> d_sel1, d_sel2;
    DeviceBuffer<double> d_pv;
};

namespace {

msv_status err_status(uint32_t err) {
    if (err & msvk::kErrBadResidue) return MSV_ERR_BAD_RESIDUE;
    if (err & msvk::kErrTooLong) return MSV_ERR_SEQUENCE_TOO_LONG;
    return err ? MSV_ERR_INVALID_ARGUMENT : MSV_OK;  // kErrBadOrder: a select entry or count outside the batch
}

// Reads (and clears when set) one error word of the profile on `st`, synchronously.
msv_status read_errors(msv_fwd_profile* p, int word, hipStream_t st) {
    uint32_t err = 0;
    MSV_HIP(hipMemcpyAsync(&err, p->d_words + word, sizeof(err), hipMemcpyDeviceToHost, st));
    MSV_HIP(hipStreamSynchronize(st));
    if (err) {
        MSV_HIP(hipMemsetAsync(p->d_words + word, 0, sizeof(uint32_t), st));
        MSV_HIP(hipStreamSynchronize(st));
    }
    return err_status(err);
}

// The variant covering `states` with the fewest slots (one per S and insert mode).
const fwdk::FwdVariant* pick_variant(uint32_t states, bool isc) {
    int n = 0;
    const fwdk::FwdVariant* all = fwdk::fwd_variants(&n);
    const fwdk::FwdVariant* best = nullptr;
    for (int i = 0; i < n; ++i) {
        const fwdk::FwdVariant& v = all[i];
        if (v.isc != isc || static_cast<uint32_t>(v.states()) < states) continue;
        if (!best || v.states() < best->states()) best = &v;
    }
    return best;
}

// Lays the variant's tables out (msv_host::fwd_tables) and uploads them, all or none.
msv_status install(msv_fwd_profile* p, const fwdk::FwdVariant* v) {
    const msv_host::FwdTables t =
        msv_host::fwd_tables(p->msc.data(), p->isc_tab.data(), p->tsc.data(), p->model_length, v->S, p->isc);
    auto upload = [](DeviceBuffer<float2>& d, const std::vector<float>& pairs) {
        return d.replace_with(reinterpret_cast<const float2*>(pairs.data()), pairs.size() / 2);
    };
    DeviceBuffer<float2> de, di, dt;
    DeviceBuffer<float> ds;
    hipError_t e;
    if ((e = upload(de, t.et)) != hipSuccess || (e = upload(dt, t.tt)) != hipSuccess ||
        (e = ds.replace_with(t.scan.data(), t.scan.size())) != hipSuccess ||
        (p->isc && (e = upload(di, t.it)) != hipSuccess))
        return hip_status(e);
    int blocks = 0;
    if ((e = msvrt::resident_blocks(p->device, v->fn, v->waves * 64, &blocks)) != hipSuccess) return hip_status(e);
    // the previous tables may still be read by a launch in flight on any stream
    if (p->d_etab || p->d_ttab) (void)hipDeviceSynchronize();
    p->d_etab = std::move(de);
    p->d_itab = std::move(di);
    p->d_ttab = std::move(dt);
    p->d_scan = std::move(ds);
    p->v = v;
    p->blocks = static_cast<uint32_t>(std::max(1, blocks));
    return MSV_OK;
}

hipStream_t stream_of(const msv_fwd_profile* p, void* stream) {
    return stream ? static_cast<hipStream_t>(stream) : static_cast<hipStream_t>(p->stream);
}

// Every launch takes the next counter slot (launch_ring.h); `errors` is the word the kernel latches its error
// bits into (device launches: kErrWord; host calls: kHostErrWord).
msv_status launch(msv_fwd_profile* p, const uint8_t* d_residues, const uint64_t* d_offsets, uint64_t n,
                  const uint32_t* d_select, const uint32_t* d_select_count, float* d_scores, hipStream_t st,
                  uint32_t* errors) {
    if (n == 0) return MSV_OK;
    if (n >= (1ull << 32)) return MSV_ERR_INVALID_ARGUMENT;
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
    // one wave per sequence: no more workgroups than the items need (a device count is bounded by n)
    const uint64_t per_block = static_cast<uint64_t>(p->v->waves);
    const uint64_t need = (n + per_block - 1) / per_block;
    const uint32_t blocks = static_cast<uint32_t>(std::min<uint64_t>(p->blocks, need));
    const bool lazy = st == p->stream || (p->bound && st == p->bound);
    MSV_HIP(p->kernels.run(st, lazy, p->d_words.get(), 2, [&](uint32_t* counter) {
        a.counter = counter;
        return fwdk::fwd_launch(*p->v, blocks, a, st);
    }));
    return MSV_OK;
}

}  // namespace

extern "C" {

void msv_fwd_profile_destroy(msv_fwd_profile* p) {
    if (!p) return;
    DeviceGuard g(p->device);
    (void)hipDeviceSynchronize();
    delete p;
}

msv_status msv_fwd_profile_reserve_length(msv_fwd_profile* p, uint64_t max_length) {
    if (!p) return MSV_ERR_INVALID_ARGUMENT;
    if (max_length >= (1ull << 31)) return MSV_ERR_SEQUENCE_TOO_LONG;
    const uint32_t need = static_cast<uint32_t>(max_length) + 1;
    if (need <= p->lentab_n) return MSV_OK;
    DeviceGuard g(p->device);
    if (!g.ok) return MSV_ERR_NO_DEVICE;
    const uint32_t n = std::max(need, p->lentab_n * 2);
    std::vector<float2> host(n);
    for (uint32_t L = 0; L < n; ++L) {
        float loop, move;
        msv_sequence_transitions(L, &loop, &move);
        host[L].x = static_cast<float>(std::exp(static_cast<double>(loop)));
        host[L].y = static_cast<float>(std::exp(static_cast<double>(move)));
    }
    MSV_HIP(p->d_lentab.replace_with(host.data(), n));
    p->lentab_n = n;
    return MSV_OK;
}

msv_status msv_fwd_profile_create(int device, const float* match_scores, const float* insert_scores,
                                  const float* transition_scores, uint32_t model_length, float tr_B_Mk, float tr_E_C,
                                  float tr_E_J, msv_fwd_profile** out) {
    if (!match_scores || !transition_scores || !out || model_length < 2) return MSV_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    // log-probabilities (msv_vit_profile_create's rule): the tolerance and the scaling rule assume odds <= 1
    for (size_t k = 1; k + 1 < model_length; ++k)
        for (int t = 0; t < 7; ++t)
            if (!(transition_scores[k * 7 + t] <= 0.0f)) return MSV_ERR_INVALID_ARGUMENT;
    const fwdk::FwdVariant* v = pick_variant(model_length - 1, insert_scores != nullptr);
    if (!v) return MSV_ERR_UNSUPPORTED_MODEL;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return MSV_ERR_NO_DEVICE;
    if (device < 0 || device >= ndev) return MSV_ERR_NO_DEVICE;
    DeviceGuard g(device);
    if (!g.ok) return MSV_ERR_NO_DEVICE;
    auto* p = new (std::nothrow) msv_fwd_profile;
    if (!p) return MSV_ERR_OUT_OF_MEMORY;
    p->device = device;
    p->model_length = model_length;
    p->isc = insert_scores != nullptr;
    p->tBM = static_cast<float>(std::exp(static_cast<double>(tr_B_Mk)));
    p->tEC = static_cast<float>(std::exp(static_cast<double>(tr_E_C)));
    p->tEJ = static_cast<float>(std::exp(static_cast<double>(tr_E_J)));
    const size_t M = model_length;
    p->msc.assign(match_scores, match_scores + 20 * M);
    if (insert_scores) p->isc_tab.assign(insert_scores, insert_scores + 20 * M);
    p->tsc.assign(transition_scores, transition_scores + 7 * M);
    hipError_t e;
    if ((e = p->stream.create(hipStreamNonBlocking)) != hipSuccess ||
        (e = p->kernels.create_events()) != hipSuccess || (e = p->d_words.reserve(kWords)) != hipSuccess ||
        (e = hipMemset(p->d_words, 0, kWords * sizeof(uint32_t))) != hipSuccess) {
        msv_fwd_profile_destroy(p);
        return hip_status(e);
    }
    msv_status s = install(p, v);
    if (s == MSV_OK) s = msv_fwd_profile_reserve_length(p, kDefaultMaxLength - 1);
    if (s != MSV_OK) {
        msv_fwd_profile_destroy(p);
        return s;
    }
    *out = p;
    return MSV_OK;
}

msv_status msv_fwd_profile_create_from_hmm(int device, const msv_hmm* hmm, int insert_mode, msv_fwd_profile** out) {
    if (!hmm || !out) return MSV_ERR_INVALID_ARGUMENT;
    const size_t M = msv_hmm_model_length(hmm);
    std::vector<float> msc(20 * M), isc(20 * M), tsc(7 * M);
    float b, c, j;
    msv_status s = msv_hmm_viterbi_scores(hmm, insert_mode, msc.data(), isc.data(), tsc.data(), &b, &c, &j);
    if (s != MSV_OK) return s;
    return msv_fwd_profile_create(device, msc.data(), insert_mode == MSV_INSERTS_LOG_ODDS ? isc.data() : nullptr,
                                  tsc.data(), static_cast<uint32_t>(M), b, c, j, out);
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
    hipFuncAttributes fa{};
    if (hipFuncGetAttributes(&fa, p->v->fn) == hipSuccess) {
        out->scratch_bytes = static_cast<uint32_t>(fa.localSizeBytes);
        out->lds_bytes = static_cast<uint32_t>(fa.sharedSizeBytes);
    }
    return MSV_OK;
}

int msv_fwd_variant_count(void) {
    int n = 0;
    fwdk::fwd_variants(&n);
    return n;
}

const char* msv_fwd_variant_name(int i) {
    int n = 0;
    const fwdk::FwdVariant* all = fwdk::fwd_variants(&n);
    return (i >= 0 && i < n) ? all[i].name : "";
}

msv_status msv_fwd_profile_set_variant(msv_fwd_profile* p, const char* name) {
    if (!p || !name) return MSV_ERR_INVALID_ARGUMENT;
    int n = 0;
    const fwdk::FwdVariant* all = fwdk::fwd_variants(&n);
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

msv_status msv_fwd_score_batch_device(msv_fwd_profile* p, const uint8_t* d_residues, uint64_t residues_len,
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

msv_status msv_fwd_profile_bind_stream(msv_fwd_profile* p, void* stream) {
    if (!p) return MSV_ERR_INVALID_ARGUMENT;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (st == p->bound) return MSV_OK;
    DeviceGuard g(p->device);
    if (!g.ok) return MSV_ERR_NO_DEVICE;
    if (p->bound) MSV_HIP(p->kernels.flush(p->bound));  // the old stream loses its guarantee
    p->bound = st;
    return MSV_OK;
}

msv_status msv_fwd_profile_check(msv_fwd_profile* p, void* stream) {
    if (!p) return MSV_ERR_INVALID_ARGUMENT;
    DeviceGuard g(p->device);
    if (!g.ok) return MSV_ERR_NO_DEVICE;
    return read_errors(p, kErrWord, stream_of(p, stream));
}

msv_status msv_fwd_score_batch(msv_fwd_profile* p, const uint8_t* residues, const uint64_t* offsets, uint64_t n,
                               float* scores, void* stream) {
    if (!p || (n && (!offsets || !scores))) return MSV_ERR_INVALID_ARGUMENT;
    if (n == 0) return MSV_OK;
    uint64_t longest = 0, total = 0;
    msv_status s = csr_extent(offsets, n, &longest, &total);
    if (s != MSV_OK) return s;
    if (total && !residues) return MSV_ERR_INVALID_ARGUMENT;
    DeviceGuard g(p->device);
    if (!g.ok) return MSV_ERR_NO_DEVICE;
    s = msv_fwd_profile_reserve_length(p, longest);
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
    if (!msv || !vit || !fwd || !stats || !n_passed_msv || !n_passed_vit ||
        (n && (!offsets || !msv_scores || !passed_msv || !vit_scores || !passed_vit || !fwd_scores || !fwd_pvalues)))
        return MSV_ERR_INVALID_ARGUMENT;
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
    uint32_t* const d_n1 = fwd->d_words + kSel1Word;
    uint32_t* const d_n2 = fwd->d_words + kSel2Word;
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
    if ((s = msv_vit_score_batch_device(vit, sg.d_res, total, sg.d_off, n, fwd->d_sel1, d_n1, fwd->d_vit_out, st)) !=
        MSV_OK)
        return s;
    // 4. P <= F2 over the Viterbi scores (a sequence that did not run has -inf, so P = 1); 5. Forward on them
    MSV_HIP(ninf_fill(sg.d_scores));
    if ((s = msv_filter_select_device(fwd->device, fwd->d_vit_out, sg.d_off, sg.d_order, n, stats[2], stats[3], F2,
                                      nullptr, fwd->d_sel2, d_n2, st)) != MSV_OK)
        return s;
    if ((s = launch(fwd, sg.d_res, sg.d_off, n, fwd->d_sel2, d_n2, sg.d_scores, st, fwd->d_words + kHostErrWord)) !=
        MSV_OK)
        return s;
    // 6. Forward P-values (a sequence that did not run has -inf: bits < tau, P = 1)
    MSV_HIP(fwdk::launch_fwd_pvalues(sg.d_scores, sg.d_off, n, stats[4], stats[5], fwd->d_pv, st));
    uint32_t counts[2] = {0, 0};
    MSV_HIP(hipMemcpyAsync(msv_scores, fwd->d_msv_out, n * sizeof(float), hipMemcpyDeviceToHost, st));
    MSV_HIP(hipMemcpyAsync(vit_scores, fwd->d_vit_out, n * sizeof(float), hipMemcpyDeviceToHost, st));
    MSV_HIP(hipMemcpyAsync(fwd_scores, sg.d_scores, n * sizeof(float), hipMemcpyDeviceToHost, st));
    MSV_HIP(hipMemcpyAsync(fwd_pvalues, fwd->d_pv, n * sizeof(double), hipMemcpyDeviceToHost, st));
    MSV_HIP(hipMemcpyAsync(counts, d_n1, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    MSV_HIP(hipStreamSynchronize(st));
    drain.disarm();
    std::fill(passed_msv, passed_msv + n, static_cast<uint8_t>(0));
    std::fill(passed_vit, passed_vit + n, static_cast<uint8_t>(0));
    std::vector<uint32_t> sel;
    const struct {
        uint32_t count;
        const uint32_t* d_sel;
        uint8_t* mask;
    } lists[2] = {{counts[0], fwd->d_sel1, passed_msv}, {counts[1], fwd->d_sel2, passed_vit}};
    for (const auto& l : lists) {
        if (!l.count) continue;
        sel.resize(l.count);
        MSV_HIP(hipMemcpyAsync(sel.data(), l.d_sel, l.count * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        MSV_HIP(hipStreamSynchronize(st));
        for (uint32_t x : sel) l.mask[x] = 1;
    }
    *n_passed_msv = counts[0];
    *n_passed_vit = counts[1];
    // every stage's word is read, so each call clears its own bits (a bad residue latches all three)
    s = msv_profile_check(msv, st);
    const msv_status vs = msv_vit_profile_check(vit, st);
    const msv_status fs = read_errors(fwd, kHostErrWord, st);
    return s != MSV_OK ? s : vs != MSV_OK ? vs : fs;
}

}  // extern "C"
