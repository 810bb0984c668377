// cal_device.cpp -- C-ABI of the calibration stage (msv.h "Calibration") on the HIP runtime.
//
// The stage owns one explicit stream and one workspace (a chunk's residues and offsets), and drives the three engines
// through their public device calls: per sample set, per chunk, the generate launch and the engine's score call into
// the set's N-float array, then one fit launch over the N scores.  Everything is enqueued on the one stream, so the
// workspace is reused chunk after chunk with no synchronisation; the host reads the three result records once, at the
// end, and only then (where asked for) the raw scores.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <new>

#include "cal_host.h"
#include "cal_kernel.h"
#include "hip_rt.h"
#include "msv.h"

using msvrt::DeviceBuffer;
using msvrt::DeviceGuard;

namespace {

hipError_t generate(const float* background, uint64_t seed, uint32_t set, uint64_t first, uint64_t n, uint64_t L,
                    uint8_t* d_codes, uint64_t* d_offsets, hipStream_t st) {
    calk::GenerateArgs a;
    a.T = msv_host::cal_thresholds(background);
    a.codes = d_codes;
    a.offsets = d_offsets;
    a.seed = seed;
    a.first = first;
    a.n = n;
    a.L = L;
    a.set = set;
    return calk::launch_generate(a, st);
}

bool generate_ok(uint64_t n, uint64_t L, const uint8_t* d_codes, const uint64_t* d_offsets) {
    if (!d_offsets || L >= (1ull << 31) || n >= msvrt::kMaxLaunchSeqs) return false;
    if (L && n > (msvrt::kChunkBytes - 1) / L) return false;
    if (n && L && (!d_codes || reinterpret_cast<uintptr_t>(d_codes) % calk::kGenerateBytes)) return false;
    return true;
}

msv_status score(uint32_t set, msv_profile* msv, msv_vit_profile* vit, msv_fwd_profile* fwd, const uint8_t* d_codes,
                 uint64_t bytes, const uint64_t* d_off, uint64_t n, float* d_scores, hipStream_t st) {
    switch (set) {
        case MSV_CAL_SET_MSV: return msv_score_batch_device(msv, d_codes, bytes, d_off, n, nullptr, d_scores, st);
        case MSV_CAL_SET_VITERBI:
            return msv_vit_score_batch_device(vit, d_codes, bytes, d_off, n, nullptr, nullptr, d_scores, st);
        default: return msv_fwd_score_batch_device(fwd, d_codes, bytes, d_off, n, nullptr, nullptr, d_scores, st);
    }
}

}  // namespace

extern "C" {

msv_status msv_cal_generate_device(int device, const float* background, uint64_t seed, uint32_t set, uint64_t first,
                                   uint64_t n, uint64_t L, uint8_t* d_codes, uint64_t* d_offsets, void* stream) {
    if (!background || !stream || !generate_ok(n, L, d_codes, d_offsets)) return MSV_ERR_INVALID_ARGUMENT;
    DeviceGuard g(device);
    if (!g.ok) return MSV_ERR_NO_DEVICE;
    MSV_HIP(generate(background, seed, set, first, n, L, d_codes, d_offsets, static_cast<hipStream_t>(stream)));
    return MSV_OK;
}

msv_status msv_cal_fit_device(int device, const float* d_scores, uint64_t n, uint64_t L, int mode, double lambda,
                              double tail, msv_cal_fit* d_record, void* stream) {
    if (!d_record || !stream || (n && !d_scores)) return MSV_ERR_INVALID_ARGUMENT;
    DeviceGuard g(device);
    if (!g.ok) return MSV_ERR_NO_DEVICE;
    calk::FitArgs a;
    a.scores = d_scores;
    a.record = d_record;
    a.n = n;
    a.L = L;
    a.lambda = lambda;
    a.tail = tail;
    a.mode = mode;
    MSV_HIP(calk::launch_fit(a, static_cast<hipStream_t>(stream)));
    return MSV_OK;
}

msv_status msv_cal_calibrate(const msv_hmm* hmm, msv_profile* msv, msv_vit_profile* vit, msv_fwd_profile* fwd,
                             const msv_cal_options* options, float* stats, msv_cal_report* report) {
    if (!hmm || !stats) return MSV_ERR_INVALID_ARGUMENT;
    const uint32_t sets = (msv ? 1u : 0u) | (vit ? 2u : 0u) | (fwd ? 4u : 0u);
    msv_host::CalPlan plan;
    if (!msv_host::cal_plan(options, sets, &plan)) return MSV_ERR_INVALID_ARGUMENT;
    const float* const bg = msv_background_frequencies();
    double lambda = 0.0;
    msv_status s = msv_cal_lambda(msv_hmm_match_emissions(hmm), static_cast<uint32_t>(msv_hmm_model_length(hmm)), bg,
                                  &lambda);
    if (s != MSV_OK) return s;
    msv_cal_fit rec[3];
    uint64_t chunks[3] = {0, 0, 0};
    std::memset(rec, 0, sizeof(rec));
    if (!sets) {
        msv_host::cal_finish(plan, sets, lambda, rec, chunks, stats, report);
        return MSV_OK;
    }

    // one device, and the engines' length tables
    int device = -1;
    const auto same_device = [&](int d) {
        if (device < 0) device = d;
        return device == d;
    };
    if (msv) {
        msv_kernel_info i;
        if ((s = msv_profile_describe(msv, &i)) != MSV_OK) return s;
        if (!same_device(i.device)) return MSV_ERR_INVALID_ARGUMENT;
        if ((s = msv_profile_reserve_length(msv, plan.L[0])) != MSV_OK) return s;
    }
    if (vit) {
        msv_vit_info i;
        if ((s = msv_vit_profile_describe(vit, &i)) != MSV_OK) return s;
        if (!same_device(i.device)) return MSV_ERR_INVALID_ARGUMENT;
        if ((s = msv_vit_profile_reserve_length(vit, plan.L[1])) != MSV_OK) return s;
    }
    if (fwd) {
        msv_fwd_info i;
        if ((s = msv_fwd_profile_describe(fwd, &i)) != MSV_OK) return s;
        if (!same_device(i.device)) return MSV_ERR_INVALID_ARGUMENT;
        if ((s = msv_fwd_profile_reserve_length(fwd, plan.L[2])) != MSV_OK) return s;
    }

    uint64_t per_chunk[3] = {0, 0, 0}, ws_bytes = 0;
    for (uint32_t set = 0; set < 3; ++set) {
        if (!(sets >> set & 1u)) continue;
        per_chunk[set] = std::min(plan.n[set], msv_host::cal_chunk_sequences(plan.workspace, plan.L[set]));
        if (per_chunk[set] == 0) return MSV_ERR_OUT_OF_MEMORY;
        ws_bytes = std::max(ws_bytes, msv_host::cal_workspace_bytes(per_chunk[set], plan.L[set]));
    }

    DeviceGuard g(device);
    if (!g.ok) return MSV_ERR_NO_DEVICE;
    msvrt::Stream stream;
    MSV_HIP(stream.create(hipStreamNonBlocking));
    const hipStream_t st = stream;
    DeviceBuffer<uint8_t> d_ws;
    DeviceBuffer<float> d_scores[3];
    DeviceBuffer<msv_cal_fit> d_rec;
    MSV_HIP(d_ws.reserve(ws_bytes));
    MSV_HIP(d_rec.reserve(3));
    for (uint32_t set = 0; set < 3; ++set)
        if (sets >> set & 1u) MSV_HIP(d_scores[set].reserve(plan.n[set]));

    msvrt::StreamDrain drain(st);  // the buffers above are freed after it on every early return
    for (uint32_t set = 0; set < 3; ++set) {
        if (!(sets >> set & 1u)) continue;
        const uint64_t N = plan.n[set], L = plan.L[set];
        for (uint64_t first = 0; first < N; first += per_chunk[set]) {
            const uint64_t cnt = std::min(per_chunk[set], N - first);
            uint8_t* const d_codes = d_ws;
            uint64_t* const d_off = reinterpret_cast<uint64_t*>(d_ws + msv_host::cal_codes_bytes(cnt, L));
            if (!generate_ok(cnt, L, d_codes, d_off)) return MSV_ERR_INVALID_ARGUMENT;
            MSV_HIP(generate(bg, plan.seed, set, first, cnt, L, d_codes, d_off, st));
            s = score(set, msv, vit, fwd, d_codes, cnt * L, d_off, cnt, d_scores[set] + first, st);
            if (s != MSV_OK) return s;
            chunks[set] += 1;
        }
        s = msv_cal_fit_device(device, d_scores[set], N, L,
                               set == MSV_CAL_SET_FORWARD ? MSV_CAL_FIT_TAU : MSV_CAL_FIT_LOCATION, lambda, plan.tail,
                               d_rec + set, st);
        if (s != MSV_OK) return s;
    }
    MSV_HIP(hipMemcpyAsync(rec, d_rec, sizeof(rec), hipMemcpyDeviceToHost, st));
    for (uint32_t set = 0; set < 3; ++set)
        if ((sets >> set & 1u) && plan.scores[set])
            MSV_HIP(hipMemcpyAsync(plan.scores[set], d_scores[set], plan.n[set] * sizeof(float), hipMemcpyDeviceToHost,
                                   st));
    MSV_HIP(hipStreamSynchronize(st));
    drain.disarm();
    if (msv && (s = msv_profile_check(msv, st)) != MSV_OK) return s;
    if (vit && (s = msv_vit_profile_check(vit, st)) != MSV_OK) return s;
    if (fwd && (s = msv_fwd_profile_check(fwd, st)) != MSV_OK) return s;
    for (uint32_t set = 0; set < 3; ++set)
        if ((sets >> set & 1u) && rec[set].status != MSV_OK) return static_cast<msv_status>(rec[set].status);
    msv_host::cal_finish(plan, sets, lambda, rec, chunks, stats, report);
    return MSV_OK;
}

}  // extern "C"
