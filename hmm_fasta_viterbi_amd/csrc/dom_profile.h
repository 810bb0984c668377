// dom_profile.h -- the domain profile's layout, shared by the two device layers that run on it: dom_device.cpp (the
// decode) and aln_device.cpp (the alignment stage, DESIGN 4.11, which adds no profile type).
#pragma once

#include <hip/hip_runtime.h>

#include "dom_kernel.h"
#include "hip_rt.h"
#include "stage_profile.h"

struct msv_dom_profile : stagedev::StageProfile {
    float tBM = 0, tEC = 0, tEJ = 0;  // odds of tr_B_Mk, tr_E_C, tr_E_J
    float tr_B_Mk = 0, tr_E_C = 0, tr_E_J = 0;  // the scores themselves (the alignment stage's gates)
    const domk::DomVariant* v = nullptr;
    msvrt::DeviceBuffer<float> d_scan;       // Forward's scan multipliers
    msvrt::DeviceBuffer<float2> d_btab;      // Backward slot arrays [8][S/2][64]
    msvrt::DeviceBuffer<float> d_bscan;      // the mirrored scan's multipliers
    uint32_t bck_blocks = 0;                 // persistent grid of a full Backward launch
    // msv_dom_decode_batch's buffers
    msvrt::DeviceBuffer<float> d_bck, d_begin, d_end, d_occ;
    msvrt::DeviceBuffer<uint32_t> d_records, d_sel, d_counts, d_rcount;
    msvrt::DeviceBuffer<uint64_t> d_rows, d_roff;
    msvrt::DeviceBuffer<msv_dom_region> d_regions;
};
