// vit_profile.h -- the Viterbi profile as the device layer's translation units see it: vit_device.cpp (scores,
// the filter pipeline) and vit_trace_device.cpp (traces) share one msv_vit_profile.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "hip_rt.h"
#include "msv.h"
#include "stage_profile.h"
#include "vit_kernel.h"

namespace vitdev {

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

// The shared stage profile (stage_profile.h) with the log-score constants, the variant, msv_vit_filter_batch's MSV
// scores and survivors list (its count: stagedev::kSelWord), the debug hooks and the trace's state.
struct msv_vit_profile : stagedev::StageProfile {
    float tr_B_Mk = 0, tr_E_C = 0, tr_E_J = 0;
    const vitk::VitVariant* v = nullptr;
    msvrt::DeviceBuffer<float> d_msc_out;
    msvrt::DeviceBuffer<uint32_t> d_sel;
    hipEvent_t time_start = nullptr, time_stop = nullptr;  // msv_vit_debug_time_next_launch
    uint64_t* d_stamps = nullptr;                          // msv_vit_debug_set_stamps (tools only)
    vitdev::TraceState trace;
};
