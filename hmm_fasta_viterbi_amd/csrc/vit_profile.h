// vit_profile.h -- the Viterbi profile as the device layer's translation units see it: vit_device.cpp (scores,
// the filter pipeline) and vit_trace_device.cpp (traces) share one msv_vit_profile.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "hip_rt.h"
#include "launch_ring.h"
#include "msv.h"
#include "vit_kernel.h"

namespace vitdev {

// d_words: [2k, 2k+1] = launch slot k's dequeue counters {next index, leavers} (zero between launches),
// [kErrWord] = sticky error bits of device launches (msv_vit_profile_check), [kHostErrWord] = the error bits
// of the synchronous host calls, which report and clear only their own, [kSelWord] = msv_vit_filter_batch's
// survivors count.
constexpr int kLaunchSlots = 8;
constexpr int kErrWord = 2 * kLaunchSlots;
constexpr int kHostErrWord = kErrWord + 1;
constexpr int kSelWord = kHostErrWord + 1;
constexpr int kWords = kSelWord + 1;

// What msv_vit_trace_batch keeps between calls (vit_trace_device.cpp): the tables in its plan's layout, built
// on the first trace, and the chunk's device buffers.
struct TraceState {
    int plan = -1;  // vit_trace_plan.h's kPlans index, -1 until the first trace
    uint32_t blocks = 0;
    msvrt::DeviceBuffer<float2> d_etab, d_itab, d_ttab;
    msvrt::DeviceBuffer<uint32_t> d_ws, d_select, d_counts;
    msvrt::DeviceBuffer<uint64_t> d_base, d_dom_off, d_ops_off;
    msvrt::DeviceBuffer<float> d_scores;
    msvrt::DeviceBuffer<msv_vit_domain> d_domains;
    msvrt::DeviceBuffer<uint8_t> d_ops;
    msvrt::Event t0, t1, t2, t3;  // fill start / end, walk start / end
};

}  // namespace vitdev

struct msv_vit_profile {
    int device = 0;
    uint32_t model_length = 0;  // LENG + 1
    bool isc = false;
    float tr_B_Mk = 0, tr_E_C = 0, tr_E_J = 0;
    std::vector<float> msc, isc_tab, tsc;  // host copies (re-laid when the variant changes)
    const vitk::VitVariant* v = nullptr;
    uint32_t blocks = 0;                // persistent grid of a full launch
    msvrt::DeviceBuffer<float2> d_etab;        // [20][S/2][64]
    msvrt::DeviceBuffer<float2> d_itab;        // [20][S/2][64] (isc)
    msvrt::DeviceBuffer<float2> d_ttab;        // [7][S/2][64]
    msvrt::DeviceBuffer<float2> d_lentab;
    uint32_t lentab_n = 0;
    msvrt::DeviceBuffer<uint32_t> d_words;     // kWords, see kLaunchSlots
    msvrt::LaunchRing<vitdev::kLaunchSlots> kernels;  // the launch slots' streams and events
    msvrt::Stream stream;
    hipStream_t bound = nullptr;        // msv_vit_profile_bind_stream: a caller stream kept alive while bound
    // msv_vit_score_batch / msv_vit_filter_batch staging (staged.d_scores: the Viterbi scores); the filter's
    // MSV scores and survivors list beside it
    msvrt::CsrStaging staged;
    msvrt::DeviceBuffer<float> d_msc_out;
    msvrt::DeviceBuffer<uint32_t> d_sel;
    hipEvent_t time_start = nullptr, time_stop = nullptr;  // msv_vit_debug_time_next_launch
    uint64_t* d_stamps = nullptr;                          // msv_vit_debug_set_stamps (tools only)
    vitdev::TraceState trace;
};

namespace vitdev {

msv_status err_status(uint32_t err);
// Reads (and clears when set) one error word of the profile on `st`, synchronously.
msv_status read_errors(msv_vit_profile* p, int word, hipStream_t st);

}  // namespace vitdev
