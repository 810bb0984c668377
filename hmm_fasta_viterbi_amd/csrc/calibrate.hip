// calibrate.hip -- the calibration stage on gfx950 (msv.h "Calibration"): the null sample and the fits.
//
//   cal_generate_kernel   one thread produces kGenerateBytes = 16 consecutive bytes of the flat code array (flat byte
//                         g is residue g % L of sequence first + g / L: the key is taken anew where a thread crosses
//                         into the next sequence) and writes them with one 16-byte vector store; the thread that holds
//                         the ragged end writes it in byte stores.  Thread t <= n also writes offsets[t] = t L.  The
//                         draw is cal_host.h's cal_residue, the function msv_cal_generate runs: integers only, so the
//                         bytes are the host's.  The 19 thresholds are kernel arguments.
//   cal_fit_kernel        ONE workgroup of kFitBlock = 256 threads, float64.  Thread t adds elements t, t + 256, .. in
//                         index order; the 256 partial values meet in an LDS tree halved 128, 64, .., 1 -- a fixed
//                         order, no atomics.  Passes over the n scores: minimum, maximum and the non-finite count;
//                         sum y; sum (y - ybar)^2; per Newton iteration S0, S1, S2 (cal_host.h's cal_newton, the
//                         host's loop, every thread running it on the same reduced values); S0 at the final lambda.
//                         Thread 0 writes the 40-byte record.  Bad input sets the record's status word: the kernel
//                         never loops on it (the Newton loop is bounded by kCalMaxIterations).
#include <hip/hip_runtime.h>

#include "cal_host.h"
#include "cal_kernel.h"

namespace calk {

using msv_host::cal_finite;

__global__ __launch_bounds__(kGenerateBlock) void cal_generate_kernel(const GenerateArgs a) {
    const uint64_t t = static_cast<uint64_t>(blockIdx.x) * kGenerateBlock + threadIdx.x;
    if (t <= a.n) a.offsets[t] = t * a.L;
    const uint64_t total = a.n * a.L, g0 = t * kGenerateBytes;
    if (g0 >= total) return;
    const uint32_t count = total - g0 < kGenerateBytes ? static_cast<uint32_t>(total - g0) : kGenerateBytes;
    uint64_t s = g0 / a.L;
    uint64_t i = g0 - s * a.L;
    uint64_t key = msv_host::cal_key(a.seed, a.set, a.first + s);
    uint32_t w[kGenerateBytes / 4] = {0, 0, 0, 0};
#pragma unroll
    for (uint32_t b = 0; b < kGenerateBytes; ++b) {
        if (b < count) {
            const uint32_t code = msv_host::cal_residue(a.T, key, static_cast<uint32_t>(i));
            w[b >> 2] |= code << (8 * (b & 3));
            if (++i == a.L) {
                i = 0;
                ++s;
                key = msv_host::cal_key(a.seed, a.set, a.first + s);
            }
        }
    }
    if (count == kGenerateBytes) {
        *reinterpret_cast<uint4*>(a.codes + g0) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
#pragma unroll
        for (uint32_t b = 0; b < kGenerateBytes; ++b)
            if (b < count) a.codes[g0 + b] = static_cast<uint8_t>(w[b >> 2] >> (8 * (b & 3)));
    }
}

namespace {

enum { kSum, kMin, kMax };

// Three values per thread through the LDS tree; every thread returns with the three results.
template <int OP0, int OP1, int OP2>
__device__ __forceinline__ void reduce3(double (&sh)[3][kFitBlock], double (&v)[3]) {
    const uint32_t t = threadIdx.x;
    auto op = [](int which, double x, double y) {
        return which == kSum ? x + y : which == kMin ? (y < x ? y : x) : (y > x ? y : x);
    };
    sh[0][t] = v[0];
    sh[1][t] = v[1];
    sh[2][t] = v[2];
    __syncthreads();
#pragma unroll
    for (uint32_t d = kFitBlock / 2; d >= 1; d >>= 1) {
        if (t < d) {
            sh[0][t] = op(OP0, sh[0][t], sh[0][t + d]);
            sh[1][t] = op(OP1, sh[1][t], sh[1][t + d]);
            sh[2][t] = op(OP2, sh[2][t], sh[2][t + d]);
        }
        __syncthreads();
    }
    v[0] = sh[0][0];
    v[1] = sh[1][0];
    v[2] = sh[2][0];
    __syncthreads();  // the next reduction rewrites sh
}

}  // namespace

__global__ __launch_bounds__(kFitBlock) void cal_fit_kernel(const FitArgs a) {
    __shared__ double sh[3][kFitBlock];
    const uint32_t t = threadIdx.x;
    const uint64_t n = a.n;
    uint32_t iterations = 0;
    auto finish = [&](msv_status status, double mu, double lambda, double gmu, double glam) {
        if (t != 0) return;
        msv_cal_fit r;
        r.mu = mu;
        r.lambda = lambda;
        r.gmu = gmu;
        r.glam = glam;
        r.iterations = iterations;
        r.status = static_cast<uint32_t>(status);
        *a.record = r;
    };
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    auto fail = [&](msv_status status) { finish(status, nan, nan, nan, nan); };

    const bool fitted = a.mode == MSV_CAL_FIT_GUMBEL || a.mode == MSV_CAL_FIT_TAU;
    const bool given = a.mode == MSV_CAL_FIT_LOCATION || a.mode == MSV_CAL_FIT_TAU;
    if (n < 2 || !(fitted || given) || (given && (!cal_finite(a.lambda) || !(a.lambda > 0.0))) ||
        (a.mode == MSV_CAL_FIT_TAU && (!cal_finite(a.tail) || !msv_host::cal_tail_ok(a.tail))))
        return fail(MSV_ERR_INVALID_ARGUMENT);

    const float nullsc = a.L ? msv_host::null1_score(a.L) : 0.0f;
    auto bits = [&](uint64_t i) { return msv_host::cal_bits(a.scores[i], a.L, nullsc); };

    double v[3] = {__longlong_as_double(0x7ff0000000000000ll), __longlong_as_double(0xfff0000000000000ll), 0.0};
    for (uint64_t i = t; i < n; i += kFitBlock) {
        const double x = bits(i);
        if (!cal_finite(a.scores[i]) || !cal_finite(x)) {
            v[2] += 1.0;
        } else {
            v[0] = x < v[0] ? x : v[0];
            v[1] = x > v[1] ? x : v[1];
        }
    }
    reduce3<kMin, kMax, kSum>(sh, v);
    const double xmin = v[0];
    if (v[2] != 0.0 || !(v[1] > xmin)) return fail(MSV_ERR_INVALID_ARGUMENT);  // not finite, or zero variance

    auto sum_exp = [&](double l) {
        double p[3] = {0.0, 0.0, 0.0};
        for (uint64_t i = t; i < n; i += kFitBlock) p[0] += exp(-l * (bits(i) - xmin));
        reduce3<kSum, kSum, kSum>(sh, p);
        return p[0];
    };

    double lambda = a.lambda;
    if (fitted) {
        double p[3] = {0.0, 0.0, 0.0};
        for (uint64_t i = t; i < n; i += kFitBlock) p[0] += bits(i) - xmin;
        reduce3<kSum, kSum, kSum>(sh, p);
        const double ybar = p[0] / static_cast<double>(n);
        p[0] = p[1] = p[2] = 0.0;
        for (uint64_t i = t; i < n; i += kFitBlock) {
            const double d = (bits(i) - xmin) - ybar;
            p[0] += d * d;
        }
        reduce3<kSum, kSum, kSum>(sh, p);
        const double var = p[0] / static_cast<double>(n - 1);
        const double lambda0 = 3.14159265358979323846 / sqrt(6.0 * var);
        const msv_status s = msv_host::cal_newton(
            ybar, lambda0,
            [&](double l, double* S) {
                double q[3] = {0.0, 0.0, 0.0};
                for (uint64_t i = t; i < n; i += kFitBlock) {
                    const double y = bits(i) - xmin;
                    const double e = exp(-l * y);
                    q[0] += e;
                    q[1] += y * e;
                    q[2] += y * y * e;
                }
                reduce3<kSum, kSum, kSum>(sh, q);
                S[0] = q[0];
                S[1] = q[1];
                S[2] = q[2];
            },
            &lambda, &iterations);
        if (s != MSV_OK) return fail(s);
    }
    const double mu = msv_host::cal_location(xmin, sum_exp(lambda), n, lambda);
    if (a.mode == MSV_CAL_FIT_TAU)
        finish(MSV_OK, msv_host::cal_tau(mu, lambda, a.lambda, a.tail), a.lambda, mu, lambda);
    else
        finish(MSV_OK, mu, lambda, mu, lambda);
}

hipError_t launch_generate(const GenerateArgs& a, hipStream_t stream) {
    const uint64_t threads = generate_threads(a.n, a.L);
    const uint64_t blocks = (threads + kGenerateBlock - 1) / kGenerateBlock;
    if (blocks >= (1ull << 31)) return hipErrorInvalidValue;
    void* params[] = {const_cast<GenerateArgs*>(&a)};
    return hipLaunchKernel(reinterpret_cast<const void*>(&cal_generate_kernel), dim3(static_cast<uint32_t>(blocks)),
                           dim3(kGenerateBlock), params, 0, stream);
}

hipError_t launch_fit(const FitArgs& a, hipStream_t stream) {
    void* params[] = {const_cast<FitArgs*>(&a)};
    return hipLaunchKernel(reinterpret_cast<const void*>(&cal_fit_kernel), dim3(1), dim3(kFitBlock), params, 0, stream);
}

}  // namespace calk
