// stage_profile.h -- what the Viterbi and the Forward device layers (vit_device.cpp, vit_trace_device.cpp,
// fwd_device.cpp) have in common: a stage's profile is one compiled variant's kernel-layout tables, a per-length
// {loop, move} table and self-resetting dequeue counters (one pair per launch slot, launch_ring.h, so one profile
// may be driven from several streams at once); a batch -- typically the previous filter's survivors, selected on
// the device -- is one persistent launch (seq_queue.h is the kernels' side).  msv_vit_profile and msv_fwd_profile
// derive from StageProfile and add their constants, their variant and their cascade's buffers; the entry points of
// both are their argument checks and one call into the bodies below, which take what differs as small callables.
// The domain profile (dom_profile.h) is a third, and the stages that run on it (dom_device.cpp, aln_device.cpp,
// spl_device.cpp) launch through run() with the grid of the kernel at hand and find their variant by find_by_shape.
// As hip_rt.h: no virtuals.  (The MSV profile, msv_device.cpp, is another shape: plans, order, chunks.)
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <new>
#include <vector>

#include "hip_rt.h"
#include "launch_ring.h"
#include "msv.h"
#include "msv_kernel.h"

namespace stagedev {

using msvrt::DeviceBuffer;
using msvrt::DeviceGuard;
using msvrt::hip_status;

// d_words: [2k, 2k+1] = launch slot k's dequeue counters {next index, leavers} (zero between launches),
// [kErrWord] = sticky error bits of device launches (*_profile_check), [kHostErrWord] = the error bits of the
// synchronous host calls, which report and clear only their own, [kSelWord], [kSel2Word] = the cascades' survivor
// counts (msv_vit_filter_batch uses the first, msv_fwd_filter_batch both).
constexpr int kLaunchSlots = 8;
constexpr int kErrWord = 2 * kLaunchSlots;
constexpr int kHostErrWord = kErrWord + 1;
constexpr int kSelWord = kHostErrWord + 1;
constexpr int kSel2Word = kSelWord + 1;
constexpr int kWords = kSel2Word + 1;
constexpr uint32_t kDefaultMaxLength = 131072;

struct StageProfile {
    int device = 0;
    uint32_t model_length = 0;  // LENG + 1
    bool isc = false;
    std::vector<float> msc, isc_tab, tsc;  // host copies of the score tables (re-laid when the variant changes)
    uint32_t blocks = 0;                   // persistent grid of a full launch
    DeviceBuffer<float2> d_etab;           // [20][S/2][64]
    DeviceBuffer<float2> d_itab;           // [20][S/2][64] (isc)
    DeviceBuffer<float2> d_ttab;           // [7 or 8][S/2][64]
    DeviceBuffer<float2> d_lentab;
    uint32_t lentab_n = 0;
    DeviceBuffer<uint32_t> d_words;             // kWords, see kLaunchSlots
    msvrt::LaunchRing<kLaunchSlots> kernels;    // the launch slots' streams and events
    msvrt::Stream stream;
    hipStream_t bound = nullptr;  // *_profile_bind_stream: a caller stream kept alive while bound
    msvrt::CsrStaging staged;     // the host calls' batch (staged.d_scores: this stage's scores)
};

inline msv_status err_status(uint32_t err) {
    if (err & msvk::kErrBadResidue) return MSV_ERR_BAD_RESIDUE;
    if (err & msvk::kErrTooLong) return MSV_ERR_SEQUENCE_TOO_LONG;
    if (err & msvk::kErrBadOrder) return MSV_ERR_INVALID_ARGUMENT;  // a select entry or count outside the batch
    if (err & msvk::kErrTeamHang) return MSV_ERR_HIP;               // (the Viterbi team kernels only)
    return err ? MSV_ERR_INVALID_ARGUMENT : MSV_OK;
}

// Reads (and clears when set) one error word of the profile on `st`, synchronously.
inline msv_status read_errors(StageProfile* p, int word, hipStream_t st) {
    uint32_t err = 0;
    MSV_HIP(hipMemcpyAsync(&err, p->d_words + word, sizeof(err), hipMemcpyDeviceToHost, st));
    MSV_HIP(hipStreamSynchronize(st));
    if (err) {
        MSV_HIP(hipMemsetAsync(p->d_words + word, 0, sizeof(uint32_t), st));
        MSV_HIP(hipStreamSynchronize(st));
    }
    return err_status(err);
}

inline hipStream_t stream_of(const StageProfile* p, void* stream) {
    return stream ? static_cast<hipStream_t>(stream) : static_cast<hipStream_t>(p->stream);
}

// Streams known to outlive a launch slot's next use, whose events LaunchRing records lazily.
inline bool lazy(const StageProfile* p, hipStream_t st) { return st == p->stream || (p->bound && st == p->bound); }

// ---- variant tables: `table` is vitk::vit_variants or fwdk::fwd_variants

template <class V>
int variant_count(const V* (*table)(int*)) {
    int n = 0;
    table(&n);
    return n;
}

template <class V>
const char* variant_name(const V* (*table)(int*), int i) {
    int n = 0;
    const V* all = table(&n);
    return (i >= 0 && i < n) ? all[i].name : "";
}

template <class V>
const V* find_by_name(const V* (*table)(int*), const char* name) {
    int n = 0;
    const V* all = table(&n);
    for (int i = 0; i < n; ++i)
        if (std::strcmp(all[i].name, name) == 0) return &all[i];
    return nullptr;
}

// The entry of a sibling stage's table with a profile's shape (align and split run on the domain stage's variant).
template <class V>
const V* find_by_shape(const V* (*table)(int*), int S, bool isc) {
    int n = 0;
    const V* all = table(&n);
    for (int i = 0; i < n; ++i)
        if (all[i].S == S && all[i].isc == isc) return &all[i];
    return nullptr;
}

// The automatic choice covering `states`: among the variants of the insert mode that `ok` admits, the fewest
// slots.  Informative insert scores need an isc variant.
template <class V, class Ok>
const V* pick(const V* (*table)(int*), uint32_t states, bool isc, Ok ok) {
    int n = 0;
    const V* all = table(&n);
    const V* best = nullptr;
    for (int i = 0; i < n; ++i) {
        const V& v = all[i];
        if (!ok(v) || v.isc != isc || static_cast<uint32_t>(v.states()) < states) continue;
        if (!best || v.states() < best->states()) best = &v;
    }
    return best;
}

template <class P, class V>
msv_status set_variant(P* p, const V* (*table)(int*), const char* name, msv_status (*install)(P*, const V*)) {
    if (!p || !name) return MSV_ERR_INVALID_ARGUMENT;
    const V* v = find_by_name(table, name);
    if (!v) return MSV_ERR_INVALID_ARGUMENT;
    if (v->isc != p->isc || static_cast<uint32_t>(v->states()) < p->model_length - 1) return MSV_ERR_UNSUPPORTED_MODEL;
    DeviceGuard g(p->device);
    if (!g.ok) return MSV_ERR_NO_DEVICE;
    return install(p, v);
}

// ---- the two install functions' common ends

inline hipError_t upload_pairs(DeviceBuffer<float2>& d, const std::vector<float>& pairs) {
    return d.replace_with(reinterpret_cast<const float2*>(pairs.data()), pairs.size() / 2);
}

// The profile adopts a variant's freshly uploaded tables (all or none) and the grid of its kernel.
inline msv_status adopt_tables(StageProfile* p, const void* kernel, int threads, DeviceBuffer<float2>& de,
                               DeviceBuffer<float2>& di, DeviceBuffer<float2>& dt) {
    int blocks = 0;
    MSV_HIP(msvrt::resident_blocks(p->device, kernel, threads, &blocks));
    // the previous tables may still be read by a launch in flight on any stream
    if (p->d_etab || p->d_ttab) (void)hipDeviceSynchronize();
    p->d_etab = std::move(de);
    p->d_itab = std::move(di);
    p->d_ttab = std::move(dt);
    p->blocks = static_cast<uint32_t>(std::max(1, blocks));
    return MSV_OK;
}

// ---- creation and destruction.  A stage's create calls check_model, check_device and its pick in its own order.

template <class P>
void close(P* p) {
    if (!p) return;
    DeviceGuard g(p->device);
    (void)hipDeviceSynchronize();
    delete p;
}

template <class P>
msv_status check_model(const float* match_scores, const float* transition_scores, uint32_t model_length, P** out) {
    if (!match_scores || !transition_scores || !out || model_length < 2) return MSV_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    // Log-probabilities only.  The Viterbi kernel leaves D(LENG) out of E, exact only while every transition it
    // reads (nodes 1 .. LENG-1, install) is <= 0 (then every D is bounded by an M of its row); Forward's
    // tolerance and scaling rule assume odds <= 1.
    for (size_t k = 1; k + 1 < model_length; ++k)
        for (int t = 0; t < 7; ++t)
            if (!(transition_scores[k * 7 + t] <= 0.0f)) return MSV_ERR_INVALID_ARGUMENT;
    return MSV_OK;
}

inline msv_status check_device(int device) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return MSV_ERR_NO_DEVICE;
    return device < 0 || device >= ndev ? MSV_ERR_NO_DEVICE : MSV_OK;
}

// A new profile on `device` with the host tables, its stream, its slots' events and zeroed words; setup(p) then
// sets the stage's constants, installs the variant and reserves the default length table.
template <class P, class Setup>
msv_status open(int device, const float* match_scores, const float* insert_scores, const float* transition_scores,
                uint32_t model_length, P** out, Setup setup) {
    DeviceGuard g(device);
    if (!g.ok) return MSV_ERR_NO_DEVICE;
    auto* p = new (std::nothrow) P;
    if (!p) return MSV_ERR_OUT_OF_MEMORY;
    p->device = device;
    p->model_length = model_length;
    p->isc = insert_scores != nullptr;
    const size_t M = model_length;
    p->msc.assign(match_scores, match_scores + 20 * M);
    if (insert_scores) p->isc_tab.assign(insert_scores, insert_scores + 20 * M);
    p->tsc.assign(transition_scores, transition_scores + 7 * M);
    hipError_t e;
    msv_status s = MSV_OK;
    if ((e = p->stream.create(hipStreamNonBlocking)) != hipSuccess ||
        (e = p->kernels.create_events()) != hipSuccess || (e = p->d_words.reserve(kWords)) != hipSuccess ||
        (e = hipMemset(p->d_words, 0, kWords * sizeof(uint32_t))) != hipSuccess)
        s = hip_status(e);
    if (s == MSV_OK) s = setup(p);
    if (s != MSV_OK) {
        close(p);
        return s;
    }
    *out = p;
    return MSV_OK;
}

// `create` is the stage's msv_*_profile_create.
template <class P>
msv_status create_from_hmm(int device, const msv_hmm* hmm, int insert_mode, P** out,
                           msv_status (*create)(int, const float*, const float*, const float*, uint32_t, float, float,
                                                float, P**)) {
    if (!hmm || !out) return MSV_ERR_INVALID_ARGUMENT;
    const size_t M = msv_hmm_model_length(hmm);
    std::vector<float> msc(20 * M), isc(20 * M), tsc(7 * M);
    float b, c, j;
    const msv_status s = msv_hmm_viterbi_scores(hmm, insert_mode, msc.data(), isc.data(), tsc.data(), &b, &c, &j);
    if (s != MSV_OK) return s;
    return create(device, msc.data(), insert_mode == MSV_INSERTS_LOG_ODDS ? isc.data() : nullptr, tsc.data(),
                  static_cast<uint32_t>(M), b, c, j, out);
}

// The per-length table up to max_length: fill(L, float2&) writes length L's {loop, move} in the stage's scale.
template <class Fill>
msv_status reserve_length(StageProfile* p, uint64_t max_length, Fill fill) {
    if (!p) return MSV_ERR_INVALID_ARGUMENT;
    if (max_length >= (1ull << 31)) return MSV_ERR_SEQUENCE_TOO_LONG;
    const uint32_t need = static_cast<uint32_t>(max_length) + 1;
    if (need <= p->lentab_n) return MSV_OK;
    DeviceGuard g(p->device);
    if (!g.ok) return MSV_ERR_NO_DEVICE;
    const uint32_t n = std::max(need, p->lentab_n * 2);
    std::vector<float2> host(n);
    for (uint32_t L = 0; L < n; ++L) fill(L, host[L]);
    MSV_HIP(p->d_lentab.replace_with(host.data(), n));
    p->lentab_n = n;
    return MSV_OK;
}

inline msv_status bind_stream(StageProfile* p, void* stream) {
    if (!p) return MSV_ERR_INVALID_ARGUMENT;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (st == p->bound) return MSV_OK;
    DeviceGuard g(p->device);
    if (!g.ok) return MSV_ERR_NO_DEVICE;
    if (p->bound) MSV_HIP(p->kernels.flush(p->bound));  // the old stream loses its guarantee
    p->bound = st;
    return MSV_OK;
}

inline msv_status check(StageProfile* p, void* stream) {
    if (!p) return MSV_ERR_INVALID_ARGUMENT;
    DeviceGuard g(p->device);
    if (!g.ok) return MSV_ERR_NO_DEVICE;
    return read_errors(p, kErrWord, stream_of(p, stream));
}

// ---- launches.  A stage's launch(p, d_residues, d_offsets, n, d_select, d_select_count, d_scores, st, errors)
// fills its kernel's arguments and calls run; `errors` is the word the kernel latches its error bits into (device
// launches: kErrWord; host calls: kHostErrWord).
template <class P>
using LaunchFn = msv_status (*)(P*, const uint8_t*, const uint64_t*, uint64_t, const uint32_t*, const uint32_t*,
                                float*, hipStream_t, uint32_t*);

// One persistent launch over n list entries, per_block of them at a time per workgroup: no more workgroups than
// the items need (a device count is bounded by n).  Every launch takes the next counter slot (a slot whose
// previous launch ran on another stream is reused only after it: launch_ring.h), so launches of one profile on
// several streams never share a counter; a slot's counters are put back to zero by the last wave of every launch,
// and a failed launch may leave them dirty, so the slot's next launch resets them explicitly (LaunchRing::run).
// enqueue(blocks, counter) launches the kernel on `st`; `grid` is the persistent grid of that kernel (the profile's
// own kernel: p->blocks).
template <class Enqueue>
msv_status run(StageProfile* p, hipStream_t st, uint64_t n, uint64_t per_block, uint32_t grid, Enqueue enqueue) {
    if (n == 0) return MSV_OK;
    if (n >= (1ull << 32)) return MSV_ERR_INVALID_ARGUMENT;
    const uint64_t need = (n + per_block - 1) / per_block;
    const uint32_t blocks = static_cast<uint32_t>(std::min<uint64_t>(grid, need));
    MSV_HIP(p->kernels.run(st, lazy(p, st), p->d_words.get(), 2,
                           [&](uint32_t* counter) { return enqueue(blocks, counter); }));
    return MSV_OK;
}
template <class Enqueue>
msv_status run(StageProfile* p, hipStream_t st, uint64_t n, uint64_t per_block, Enqueue enqueue) {
    return run(p, st, n, per_block, p->blocks, enqueue);
}

template <class P>
msv_status score_batch_device(P* p, const uint8_t* d_residues, uint64_t residues_len, const uint64_t* d_offsets,
                              uint64_t n, const uint32_t* d_select, const uint32_t* d_select_count, float* d_scores,
                              void* stream, LaunchFn<P> launch) {
    if (!p || (n && (!d_offsets || !d_scores))) return MSV_ERR_INVALID_ARGUMENT;
    if (n && residues_len && !d_residues) return MSV_ERR_INVALID_ARGUMENT;
    if (d_select_count && !d_select) return MSV_ERR_INVALID_ARGUMENT;
    DeviceGuard g(p->device);
    if (!g.ok) return MSV_ERR_NO_DEVICE;
    return launch(p, d_residues, d_offsets, n, d_select, d_select_count, d_scores, stream_of(p, stream),
                  p->d_words + kErrWord);
}

// The synchronous host call: `reserve` is the stage's msv_*_profile_reserve_length.
template <class P>
msv_status score_batch_host(P* p, const uint8_t* residues, const uint64_t* offsets, uint64_t n, float* scores,
                            void* stream, msv_status (*reserve)(P*, uint64_t), LaunchFn<P> launch) {
    if (!p || (n && (!offsets || !scores))) return MSV_ERR_INVALID_ARGUMENT;
    if (n == 0) return MSV_OK;
    uint64_t longest = 0, total = 0;
    msv_status s = msvrt::csr_extent(offsets, n, &longest, &total);
    if (s != MSV_OK) return s;
    if (total && !residues) return MSV_ERR_INVALID_ARGUMENT;
    DeviceGuard g(p->device);
    if (!g.ok) return MSV_ERR_NO_DEVICE;
    s = reserve(p, longest);
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

// A cascade's tail, once `st` has been synchronised and `count` read: mask[0 .. n) = 1 at the d_sel[0 .. count)
// survivors, 0 elsewhere.
inline msv_status survivor_mask(hipStream_t st, uint32_t count, const uint32_t* d_sel, uint8_t* mask, uint64_t n) {
    std::fill(mask, mask + n, static_cast<uint8_t>(0));
    if (!count) return MSV_OK;
    std::vector<uint32_t> sel(count);
    MSV_HIP(hipMemcpyAsync(sel.data(), d_sel, count * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    MSV_HIP(hipStreamSynchronize(st));
    for (uint32_t x : sel) mask[x] = 1;
    return MSV_OK;
}

}  // namespace stagedev
