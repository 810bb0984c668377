// bias_filter_device.cpp -- C-ABI of the bias filter (msv.h "Bias filter") on the HIP runtime.
//
// A msv_bf_profile is a stage profile (stage_profile.h: launch slots, streams, error words, the host calls'
// staging) whose only table is the 26 floats of bias_filter_host.h; it has no variants and no length table.  A
// batch -- in the cascade, the MSV filter's survivors, selected on the device -- is one persistent launch of
// bias_filter.hip.  The entry points are their argument checks and one call into stage_profile.h.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <new>

#include "bias_filter_device.h"
#include "bias_filter_host.h"
#include "bias_filter_kernel.h"
#include "hip_rt.h"
#include "msv.h"
#include "msv_kernel.h"
#include "stage_profile.h"

using msvrt::DeviceBuffer;
using msvrt::DeviceGuard;
using msvrt::hip_status;

// The shared stage profile (its score tables and length table stay empty) with the device table and the
// cascade's buffers: the bias of a batch and the filtered survivor list (its count: stagedev::kSelWord).
struct msv_bf_profile : stagedev::StageProfile {
    float table[msv_host::kBfTableFloats] = {};
    DeviceBuffer<float> d_table;
    DeviceBuffer<float> d_bias;
    DeviceBuffer<uint32_t> d_sel;
};

namespace {

msv_status launch(msv_bf_profile* p, const uint8_t* d_residues, const uint64_t* d_offsets, uint64_t n,
                  const uint32_t* d_select, const uint32_t* d_select_count, float* d_scores, hipStream_t st,
                  uint32_t* errors) {
    bfk::BfArgs a{};
    a.table = p->d_table;
    a.residues = d_residues;
    a.offsets = d_offsets;
    a.select = d_select;
    a.select_count = d_select ? d_select_count : nullptr;
    a.scores = d_scores;
    a.errors = errors;
    a.n = n;
    // one wave per sequence
    return stagedev::run(p, st, n, static_cast<uint64_t>(bfk::kWaves), [&](uint32_t blocks, uint32_t* counter) {
        a.counter = counter;
        return bfk::bf_launch(blocks, a, st);
    });
}

// (no length table: every length is served)
msv_status reserve_nothing(msv_bf_profile*, uint64_t) { return MSV_OK; }

}  // namespace

namespace bfdev {

msv_status cascade_buffers(msv_bf_profile* p, uint64_t n, float** d_bias, uint32_t** d_sel, uint32_t** d_count) {
    if (!p) return MSV_ERR_INVALID_ARGUMENT;
    MSV_HIP(p->d_bias.reserve(n));
    MSV_HIP(p->d_sel.reserve(n));
    *d_bias = p->d_bias;
    *d_sel = p->d_sel;
    *d_count = p->d_words + stagedev::kSelWord;
    return MSV_OK;
}

int device_of(const msv_bf_profile* p) { return p ? p->device : -1; }

}  // namespace bfdev

extern "C" {

void msv_bf_profile_destroy(msv_bf_profile* p) { stagedev::close(p); }

msv_status msv_bf_profile_create(int device, const float* compo, const float* background, uint32_t model_length,
                                 msv_bf_profile** out) {
    if (!out) return MSV_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    msv_host::BfModel m;
    float table[msv_host::kBfTableFloats];
    msv_status s = msv_host::bf_model(compo, background, model_length, &m);
    if (s == MSV_OK) s = msv_host::bf_device_table(m, table);
    if (s == MSV_OK) s = stagedev::check_device(device);
    if (s != MSV_OK) return s;
    DeviceGuard g(device);
    if (!g.ok) return MSV_ERR_NO_DEVICE;
    auto* p = new (std::nothrow) msv_bf_profile;
    if (!p) return MSV_ERR_OUT_OF_MEMORY;
    p->device = device;
    p->model_length = model_length;
    std::memcpy(p->table, table, sizeof(table));
    int blocks = 0;
    hipError_t e;
    if ((e = p->stream.create(hipStreamNonBlocking)) != hipSuccess ||
        (e = p->kernels.create_events()) != hipSuccess || (e = p->d_words.reserve(stagedev::kWords)) != hipSuccess ||
        (e = hipMemset(p->d_words, 0, stagedev::kWords * sizeof(uint32_t))) != hipSuccess ||
        (e = p->d_table.replace_with(table, msv_host::kBfTableFloats)) != hipSuccess ||
        (e = msvrt::resident_blocks(device, bfk::bf_kernel(), bfk::kWaves * 64, &blocks)) != hipSuccess) {
        stagedev::close(p);
        return hip_status(e);
    }
    p->blocks = static_cast<uint32_t>(blocks > 0 ? blocks : 1);
    *out = p;
    return MSV_OK;
}

msv_status msv_bf_profile_create_from_hmm(int device, const msv_hmm* hmm, msv_bf_profile** out) {
    if (!hmm || !out) return MSV_ERR_INVALID_ARGUMENT;
    return msv_bf_profile_create(device, msv_hmm_compo(hmm), msv_background_frequencies(),
                                 static_cast<uint32_t>(msv_hmm_model_length(hmm)), out);
}

msv_status msv_bf_profile_describe(const msv_bf_profile* p, msv_bf_info* out) {
    if (!p || !out) return MSV_ERR_INVALID_ARGUMENT;
    std::memset(out, 0, sizeof(*out));
    out->struct_size = sizeof(*out);
    out->model_length = p->model_length;
    out->residues_per_lane = bfk::kChunk;
    out->residues_per_trip = bfk::kTrip;
    out->waves_per_block = bfk::kWaves;
    out->blocks = p->blocks;
    out->device = p->device;
    std::memcpy(out->table, p->table, sizeof(p->table));
    std::snprintf(out->variant, sizeof(out->variant), "bf_c%d_w%d", bfk::kChunk, bfk::kWaves);
    msvrt::kernel_footprint(bfk::bf_kernel(), &out->scratch_bytes, &out->lds_bytes, &out->vgprs);
    return MSV_OK;
}

msv_status msv_bf_score_batch_device(msv_bf_profile* p, const uint8_t* d_residues, uint64_t residues_len,
                                     const uint64_t* d_offsets, uint64_t n, const uint32_t* d_select,
                                     const uint32_t* d_select_count, float* d_bias, void* stream) {
    return stagedev::score_batch_device(p, d_residues, residues_len, d_offsets, n, d_select, d_select_count, d_bias,
                                        stream, launch);
}

msv_status msv_bf_profile_bind_stream(msv_bf_profile* p, void* stream) { return stagedev::bind_stream(p, stream); }

msv_status msv_bf_profile_check(msv_bf_profile* p, void* stream) { return stagedev::check(p, stream); }

msv_status msv_bf_score_batch(msv_bf_profile* p, const uint8_t* residues, const uint64_t* offsets, uint64_t n,
                              float* bias, void* stream) {
    return stagedev::score_batch_host(p, residues, offsets, n, bias, stream, reserve_nothing, launch);
}

msv_status msv_bf_filter_select_device(int device, const float* d_scores, const float* d_bias,
                                       const uint64_t* d_offsets, const uint32_t* d_order, uint64_t n, float mu,
                                       float lambda, double threshold, double* d_pvalues, uint32_t* d_selected,
                                       uint32_t* d_count, void* stream) {
    if (!d_count || (n && (!d_scores || !d_bias || !d_offsets || !d_selected))) return MSV_ERR_INVALID_ARGUMENT;
    if (n >= (1ull << 32)) return MSV_ERR_INVALID_ARGUMENT;
    // no default stream, as msv_filter_select_device
    if (!stream) return MSV_ERR_INVALID_ARGUMENT;
    DeviceGuard g(device);
    if (!g.ok) return MSV_ERR_NO_DEVICE;
    return hip_status(bfk::launch_bf_select(d_scores, d_bias, d_offsets, d_order, n, mu, lambda, threshold, d_pvalues,
                                            d_selected, d_count, static_cast<hipStream_t>(stream)));
}

msv_status msv_bf_pvalues_device(int device, const float* d_scores, const float* d_bias, const uint64_t* d_offsets,
                                 uint64_t n, float location, float scale, int kind, double* d_pvalues, void* stream) {
    if (kind != MSV_BF_GUMBEL && kind != MSV_BF_EXPONENTIAL) return MSV_ERR_INVALID_ARGUMENT;
    if (n == 0) return MSV_OK;
    if (!d_scores || !d_bias || !d_offsets || !d_pvalues) return MSV_ERR_INVALID_ARGUMENT;
    DeviceGuard g(device);
    if (!g.ok) return MSV_ERR_NO_DEVICE;
    MSV_HIP(bfk::launch_bf_pvalues(d_scores, d_bias, d_offsets, n, location, scale, kind, d_pvalues,
                                   static_cast<hipStream_t>(stream)));
    return MSV_OK;
}

}  // extern "C"
