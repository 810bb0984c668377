// cal_host.h -- host-only half of the calibration stage (msv.h "Calibration"): THE definition of the
// null sample (its key, its draw and its thresholds, which calibrate.hip's generate kernel runs too and reproduces
// byte for byte), the fits' arithmetic that the fit kernel shares (the bit score, the Newton loop, tau), the host fits
// and the CPU twin of the whole stage.  No HIP include: cal_host.cpp is built by plain g++ and runs under the
// sanitizers (tests/cpp/sanitize_calibrate.cpp).
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "fwd_host.h"
#include "msv.h"
#include "spl_host.h"  // spl_mix, kSplGolden, spl_rand24: the split stage's random numbers, unchanged

namespace msv_host {

constexpr int kCalThresholds = 19;
constexpr uint32_t kCalMaxIterations = 100;
constexpr double kCalStop = 1e-9;
constexpr uint64_t kCalDefaultN[3] = {200, 200, 200};
constexpr uint64_t kCalDefaultL[3] = {200, 200, 100};
constexpr double kCalDefaultTail = 0.04;
constexpr uint64_t kCalDefaultSeed = 42;
constexpr uint64_t kCalDefaultWorkspace = 256ull << 20;

// The thresholds travel to the kernel by value.
struct CalThresholds {
    uint32_t t[kCalThresholds];
};
// T[j] = floor(2^24 (f[0] + .. + f[j]) / (f[0] + .. + f[19])), float64, sums in index order.
CalThresholds cal_thresholds(const float* background);

// The key of sequence s of a sample set: chained as spl_key chains its fields.
FWD_HD inline uint64_t cal_key(uint64_t seed, uint32_t set, uint64_t s) {
    uint64_t h = seed;
    h = spl_mix(h + kSplGolden + set);
    h = spl_mix(h + kSplGolden + s);
    return h;
}
// The code of one 24-bit draw: the number of thresholds it reaches.
FWD_HD inline uint8_t cal_code(const CalThresholds& T, uint32_t u) {
    uint32_t c = 0;
    for (int j = 0; j < kCalThresholds; ++j) c += u >= T.t[j] ? 1u : 0u;
    return static_cast<uint8_t>(c);
}
FWD_HD inline uint8_t cal_residue(const CalThresholds& T, uint64_t key, uint32_t i) {
    return cal_code(T, spl_rand24(key, i));
}

// The bit score the fits run on (msv.h): fwd_host.h's float expressions; nullsc is null1_score(L), taken once.
// L = 0: the score is a bit score already.
FWD_HD inline double cal_bits(float score, uint64_t L, float nullsc) {
    return static_cast<double>(L ? bits_of(score - nullsc) : score);
}
// By the bits: the device objects are built with -fno-honor-nans, under which a floating-point test may be folded.
FWD_HD inline bool cal_finite(double x) {
    union {
        double d;
        uint64_t u;
    } b;
    b.d = x;
    return (b.u & 0x7ff0000000000000ull) != 0x7ff0000000000000ull;
}
FWD_HD inline bool cal_finite(float x) {
    union {
        float f;
        uint32_t u;
    } b;
    b.f = x;
    return (b.u & 0x7f800000u) != 0x7f800000u;
}

// Newton's loop of the complete fit (msv.h states it).  sums(l, S) fills S[p] = sum y_i^p exp(-l y_i), p = 0, 1, 2:
// the host's serial sums or the fit kernel's workgroup reduction (every thread then runs this loop on the same
// values).  Returns MSV_OK with *lambda the final value, or MSV_ERR_NO_CONVERGENCE.
template <class Sums>
FWD_HD inline msv_status cal_newton(double ybar, double lambda0, Sums sums, double* lambda, uint32_t* iterations) {
    double l = lambda0;
    *iterations = 0;
    for (uint32_t it = 0; it < kCalMaxIterations; ++it) {
        if (!cal_finite(l) || !(l > 0.0)) break;
        double S[3];
        sums(l, S);
        const double r = S[1] / S[0];
        const double f = 1.0 / l - ybar + r;
        const double df = r * r - S[2] / S[0] - 1.0 / (l * l);
        const double step = f / df;
        *iterations = it + 1;
        if (!cal_finite(step)) break;
        const double moved = l - step;
        const bool done = fabs(step) <= kCalStop * l;
        l = moved > 0.0 ? moved : 0.5 * l;
        if (done) {
            *lambda = l;
            return MSV_OK;
        }
    }
    return MSV_ERR_NO_CONVERGENCE;
}
// mu of the location formula from S0 = sum exp(-lambda y_i).
FWD_HD inline double cal_location(double xmin, double S0, uint64_t n, double lambda) {
    return xmin - log(S0 / static_cast<double>(n)) / lambda;
}
FWD_HD inline double cal_tau(double gmu, double glam, double lambda, double tail) {
    return gmu - log(-log(1.0 - tail)) / glam + log(tail) / lambda;
}
FWD_HD inline bool cal_tail_ok(double tail) { return tail > 0.0 && tail < 1.0; }

// Device bytes of a chunk (msv.h, msv_cal_workspace_bytes): the offsets start at the 16-byte boundary after the codes.
constexpr uint64_t cal_codes_bytes(uint64_t n, uint64_t L) { return (n * L + 15) / 16 * 16; }
constexpr uint64_t cal_workspace_bytes(uint64_t n, uint64_t L) { return cal_codes_bytes(n, L) + 8 * (n + 1); }
// The largest chunk of sequences of length L >= 1 that fits `budget` bytes, the engines' residue limit per call and
// their sequence limit; 0 where not even one fits.
uint64_t cal_chunk_sequences(uint64_t budget, uint64_t L);

// The options with every default filled in (NULL = all defaults); false where struct_size is too small or a value is
// out of range (n < 2, L outside 1 .. 2^31 - 1, a tail outside (0, 1)) for a set that runs.
struct CalPlan {
    uint64_t n[3], L[3];
    double tail;
    uint64_t seed, workspace;
    int insert_mode;
    float* scores[3];
};
bool cal_plan(const msv_cal_options* options, uint32_t sets, CalPlan* plan);
// The report and the six floats from the three records (a record is read only where its set ran).
void cal_finish(const CalPlan& plan, uint32_t sets, double lambda, const msv_cal_fit* records, const uint64_t* chunks,
                float* stats, msv_cal_report* report);

}  // namespace msv_host
