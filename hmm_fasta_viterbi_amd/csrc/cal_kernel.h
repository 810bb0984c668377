// cal_kernel.h -- device-side interface of the calibration stage, shared by calibrate.hip and the
// C-ABI layer (cal_device.cpp).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "cal_host.h"
#include "msv.h"

namespace calk {

constexpr int kGenerateBlock = 256;  // threads; each writes kGenerateBytes consecutive code bytes
constexpr int kGenerateBytes = 16;
constexpr int kFitBlock = 256;       // W: the fit's single workgroup (msv.h states its order of summation)

// cal_generate_kernel: the flat code array of sequences first .. first + n - 1 (flat byte g is residue g % L of
// sequence first + g / L) and the n + 1 offsets 0, L, 2 L, ..  codes is 16-byte aligned; n L < 2^32.
struct GenerateArgs {
    msv_host::CalThresholds T;
    uint8_t* codes;
    uint64_t* offsets;
    uint64_t seed, first, n, L;
    uint32_t set;
};
// Threads of a launch: one per 16 code bytes and at least one per offset.
constexpr uint64_t generate_threads(uint64_t n, uint64_t L) {
    const uint64_t by_codes = (n * L + kGenerateBytes - 1) / kGenerateBytes;
    return by_codes > n + 1 ? by_codes : n + 1;
}
hipError_t launch_generate(const GenerateArgs& a, hipStream_t stream);

// cal_fit_kernel: one workgroup of kFitBlock threads over n float scores.
struct FitArgs {
    const float* scores;
    msv_cal_fit* record;
    uint64_t n, L;
    double lambda, tail;
    int mode;  // msv_cal_fit_mode
};
hipError_t launch_fit(const FitArgs& a, hipStream_t stream);

}  // namespace calk
