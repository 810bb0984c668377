// bias_filter.hip -- the bias filter (msv.h "Bias filter") as ONE persistent gfx950 kernel per batch:
// HMMER3's composition filter, the Forward score of a two-state HMM (background / the profile's composition) over
// each sequence, and the filtered P-value kernels that put it between null1 and the bits of a filter stage.
//
// With T = {t00 t01; t10 t11}, D(x) = diag(1, r[x]) and pi = (pi0, pi1), the row after residue i is
//     v_1 = pi D(x_1),   v_i = v_{i-1} T D(x_i),   bias = log(v_L[0] + v_L[1])
// so v_L = pi D(x_1) (T D(x_2)) .. (T D(x_L)): a product of 2x2 matrices, which is associative.  One sequence per
// 64-lane wave on seq_queue.h's work queue (persistent grid, select / select_count, error bits).  A trip covers
// kTrip = 1,024 residues COUNTED FROM THE SEQUENCE'S FIRST RESIDUE: lane l multiplies the step matrices of residues
// trip + 16 l .. trip + 16 l + 15 in order (one unaligned 16-byte load; the last, partial chunk of a sequence byte
// by byte, never past its end), normalises its product by the power of two of its largest entry, then a six-level
// butterfly (lane ^ 1, 2, .. 32: ds_bpermute, no LDS round trip) multiplies the 64 lane products in lane order --
// at each level the lane with the level's bit clear holds the left factor, so both partners form the same product
// bit for bit -- normalising after every level; the wave's row vector then takes the trip's matrix.  Exponents are
// carried as integers.  The cuts depend on the position in the sequence only, never on its address, so a bias is a
// function of the sequence and the profile alone: not of the batch, the alignment, the select list or the stream.
// Float32 without contraction; every term is non-negative, so no step cancels.  DESIGN 4.13 counts the roundings.
#include <hip/hip_runtime.h>

#include "bias_filter_host.h"
#include "bias_filter_kernel.h"
#include "msv_kernel.h"
#include "seq_queue.h"

namespace bfk {

namespace {

// Scales four non-negative floats, the largest a positive normal number, by the power of two that brings the
// largest into [1, 2); returns its exponent.  Exact: no entry is small enough to leave the normal range (DESIGN
// 4.13's ratio bound).
__device__ __forceinline__ int normalise(float& a, float& b, float& c, float& d) {
    const float top = fmaxf(fmaxf(a, b), fmaxf(c, d));
    const int e = static_cast<int>((__float_as_uint(top) >> 23) & 0xffu) - 127;
    const float s = __uint_as_float(static_cast<uint32_t>(127 - e) << 23);
    a *= s;
    b *= s;
    c *= s;
    d *= s;
    return e;
}

}  // namespace

__global__ __launch_bounds__(kWaves * 64) void bias_filter_kernel(const BfArgs a) {
    __shared__ float r_s[20];
    __shared__ uint32_t exited_s;
    const int lane = threadIdx.x & 63;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t total = seqq::list_total(a);
    if (seqq::no_item<kWaves>(total)) {
        if (threadIdx.x == 0) seqq::count_leavers<1, 1>(a.counter);
        return;
    }
    // the 20 odds in LDS: 20 words in 20 banks, so a lookup by residue never conflicts
    if (threadIdx.x < 20) r_s[threadIdx.x] = a.table[msv_host::kBfTableR + threadIdx.x];
    if (threadIdx.x == 0) exited_s = 0;
    __syncthreads();
    const float t00 = a.table[0], t01 = a.table[1], t10 = a.table[2], t11 = a.table[3];
    const float pi0 = a.table[msv_host::kBfTablePi], pi1 = a.table[msv_host::kBfTablePi + 1];

    const uint32_t nwaves = gridDim.x * kWaves;
    uint32_t item = blockIdx.x * kWaves + wave;
    while (item < total) {
        const uint32_t s = __builtin_amdgcn_readfirstlane(a.select ? a.select[item] : item);
        if (s >= a.n) {  // an entry outside the batch is reported and never dereferenced
            if (lane == 0) atomicOr(a.errors, msvk::kErrBadOrder);
        } else {
            const uint64_t o0 = seqq::u64first(a.offsets[s]);
            const uint64_t L = seqq::u64first(a.offsets[s + 1]) - o0;
            const uint8_t* res = a.residues + o0;
            float v0 = pi0, v1 = pi1;  // the row vector is (v0, v1) * 2^ev, wave-uniform
            int ev = 0;
            bool bad = false;
            for (uint64_t trip = 0; trip < L; trip += kTrip) {
                // this lane's chunk: residues p0 .. p0 + cnt - 1, all inside the sequence
                const uint64_t p0 = trip + static_cast<uint64_t>(lane) * kChunk;
                uint32_t w[4] = {0u, 0u, 0u, 0u};
                int cnt = 0;
                if (p0 + kChunk <= L) {
                    __builtin_memcpy(w, res + p0, kChunk);
                    cnt = kChunk;
                } else if (p0 < L) {
                    cnt = static_cast<int>(L - p0);
#pragma unroll
                    for (int j = 0; j < kChunk - 1; ++j)  // (static indices keep w in registers)
                        if (j < cnt) w[j >> 2] |= static_cast<uint32_t>(res[p0 + j]) << (8 * (j & 3));
                }
                // the sequence's first residue has no transition before it: its step is D(x_1) alone
                const bool head = p0 == 0;
                float m00 = 1.0f, m01 = 0.0f, m10 = 0.0f, m11 = 1.0f;
#pragma unroll
                for (int j = 0; j < kChunk; ++j) {
                    if (j < cnt) {
                        const bool h = j == 0 && head;
                        const float c00 = h ? 1.0f : t00, c01 = h ? 0.0f : t01, c10 = h ? 0.0f : t10,
                                    c11 = h ? 1.0f : t11;
                        const uint32_t x = (w[j >> 2] >> (8 * (j & 3))) & 0xffu;
                        bad |= x >= 20u;
                        const float r = r_s[x < 20u ? x : 0u];
                        const float a0 = m00 * c00 + m01 * c10, a1 = (m00 * c01 + m01 * c11) * r;
                        const float b0 = m10 * c00 + m11 * c10, b1 = (m10 * c01 + m11 * c11) * r;
                        m00 = a0;
                        m01 = a1;
                        m10 = b0;
                        m11 = b1;
                    }
                }
                int e = normalise(m00, m01, m10, m11);
                // the 64 lane products in lane order
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
                    const float o00 = __shfl_xor(m00, d, 64), o01 = __shfl_xor(m01, d, 64);
                    const float o10 = __shfl_xor(m10, d, 64), o11 = __shfl_xor(m11, d, 64);
                    const int oe = __shfl_xor(e, d, 64);
                    const bool left = (lane & d) == 0;  // this lane's factor comes first
                    const float l00 = left ? m00 : o00, l01 = left ? m01 : o01, l10 = left ? m10 : o10,
                                l11 = left ? m11 : o11;
                    const float r00 = left ? o00 : m00, r01 = left ? o01 : m01, r10 = left ? o10 : m10,
                                r11 = left ? o11 : m11;
                    m00 = l00 * r00 + l01 * r10;
                    m01 = l00 * r01 + l01 * r11;
                    m10 = l10 * r00 + l11 * r10;
                    m11 = l10 * r01 + l11 * r11;
                    e += oe;
                    e += normalise(m00, m01, m10, m11);
                }
                // the row vector takes the trip's matrix
                float n0 = v0 * m00 + v1 * m10, n1 = v0 * m01 + v1 * m11, z0 = 0.0f, z1 = 0.0f;
                ev += e + normalise(n0, n1, z0, z1);
                v0 = n0;
                v1 = n1;
            }
            const bool any_bad = __builtin_amdgcn_ballot_w64(bad) != 0;
            if (lane == 0) {
                if (L == 0) {
                    a.scores[s] = 0.0f;
                } else if (any_bad) {
                    a.scores[s] = __builtin_inff();
                    atomicOr(a.errors, msvk::kErrBadResidue);
                } else {
                    // float64 for the one logarithm of a sequence: a single rounding to float32 is left
                    a.scores[s] = static_cast<float>(log(static_cast<double>(v0 + v1)) +
                                                     static_cast<double>(ev) * 0.69314718055994530942);
                }
            }
        }
        item = seqq::next_item(a.counter, lane, nwaves);
    }
    seqq::last_exit<kWaves>(a.counter, &exited_s, lane);
}

const void* bf_kernel() { return reinterpret_cast<const void*>(&bias_filter_kernel); }

hipError_t bf_launch(uint32_t blocks, const BfArgs& args, hipStream_t stream) {
    void* params[] = {const_cast<BfArgs*>(&args)};
    return hipLaunchKernel(bf_kernel(), dim3(blocks), dim3(kWaves * 64), params, 0, stream);
}

// ------------------------------------------------------------------------------------------------
// The filtered survivor selection: vit_kernel.hip's three launches (count per block, scan the counts, write at
// the block's prefix: a stable compaction in `order`) with the bias in the P-value.
// ------------------------------------------------------------------------------------------------
namespace {
constexpr int kSelBlock = 256;
constexpr int kScanBlock = 1024;

__device__ __forceinline__ bool select_pass(const float* scores, const float* bias, const uint64_t* offsets,
                                            const uint32_t* order, uint64_t n, float mu, float lambda,
                                            double threshold, double* pvalues, uint64_t pos, uint32_t* idx) {
    if (pos >= n) return false;
    const uint64_t i = order ? order[pos] : pos;  // (a permutation: every sequence is visited once)
    *idx = static_cast<uint32_t>(i);
    if (i >= n) return false;  // a poisoned order entry selects nothing and reads nothing
    const double p = msv_host::bf_gumbel_pvalue(scores[i], bias[i], offsets[i + 1] - offsets[i], mu, lambda);
    if (pvalues) pvalues[i] = p;
    return p <= threshold;
}
}  // namespace

__global__ __launch_bounds__(kSelBlock) void bf_select_count_kernel(const float* __restrict__ scores,
                                                                    const float* __restrict__ bias,
                                                                    const uint64_t* __restrict__ offsets,
                                                                    const uint32_t* __restrict__ order, uint64_t n,
                                                                    float mu, float lambda, double threshold,
                                                                    double* __restrict__ pvalues,
                                                                    uint32_t* __restrict__ block_counts) {
    __shared__ uint32_t lds4[4];
    uint32_t idx = 0;
    const uint64_t pos = static_cast<uint64_t>(blockIdx.x) * kSelBlock + threadIdx.x;
    const bool pass = select_pass(scores, bias, offsets, order, n, mu, lambda, threshold, pvalues, pos, &idx);
    const uint64_t mask = __builtin_amdgcn_ballot_w64(pass);
    if ((threadIdx.x & 63) == 0) lds4[threadIdx.x >> 6] = static_cast<uint32_t>(__popcll(mask));
    __syncthreads();
    if (threadIdx.x == 0) block_counts[blockIdx.x] = lds4[0] + lds4[1] + lds4[2] + lds4[3];
}

// Exclusive prefix sums of the block counts in place, and the total into *count: one workgroup, each thread a
// contiguous run of the counts.
__global__ __launch_bounds__(kScanBlock) void bf_select_scan_kernel(uint32_t* __restrict__ block_counts,
                                                                    uint32_t blocks, uint32_t* __restrict__ count) {
    __shared__ uint32_t part_s[kScanBlock];
    const uint32_t per = (blocks + kScanBlock - 1) / kScanBlock;
    const uint32_t b0 = threadIdx.x * per < blocks ? threadIdx.x * per : blocks;
    const uint32_t b1 = b0 + per < blocks ? b0 + per : blocks;
    uint32_t sum = 0;
    for (uint32_t j = b0; j < b1; ++j) sum += block_counts[j];
    part_s[threadIdx.x] = sum;
    __syncthreads();
    for (int d = 1; d < kScanBlock; d <<= 1) {
        const uint32_t v = threadIdx.x >= static_cast<uint32_t>(d) ? part_s[threadIdx.x - d] : 0u;
        __syncthreads();
        part_s[threadIdx.x] += v;
        __syncthreads();
    }
    uint32_t run = part_s[threadIdx.x] - sum;  // exclusive
    for (uint32_t j = b0; j < b1; ++j) {
        const uint32_t c = block_counts[j];
        block_counts[j] = run;
        run += c;
    }
    if (threadIdx.x == kScanBlock - 1) *count = part_s[kScanBlock - 1];
}

__global__ __launch_bounds__(kSelBlock) void bf_select_write_kernel(const float* __restrict__ scores,
                                                                    const float* __restrict__ bias,
                                                                    const uint64_t* __restrict__ offsets,
                                                                    const uint32_t* __restrict__ order, uint64_t n,
                                                                    float mu, float lambda, double threshold,
                                                                    const uint32_t* __restrict__ block_prefix,
                                                                    uint32_t* __restrict__ select) {
    __shared__ uint32_t wave_base[4];
    uint32_t idx = 0;
    const uint64_t pos = static_cast<uint64_t>(blockIdx.x) * kSelBlock + threadIdx.x;
    const bool pass = select_pass(scores, bias, offsets, order, n, mu, lambda, threshold, nullptr, pos, &idx);
    const uint64_t mask = __builtin_amdgcn_ballot_w64(pass);
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint32_t below = __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(mask >> 32),
                                                     __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(mask), 0u));
    if (lane == 0) wave_base[wv] = static_cast<uint32_t>(__popcll(mask));
    __syncthreads();
    uint32_t base = block_prefix[blockIdx.x];
    for (uint32_t k = 0; k < wv; ++k) base += wave_base[k];
    // (the passes of one launch number at most n: base + below < n, inside the caller's n entries)
    if (pass) select[base + below] = idx;
}

hipError_t launch_bf_select(const float* scores, const float* bias, const uint64_t* offsets, const uint32_t* order,
                            uint64_t n, float mu, float lambda, double threshold, double* pvalues, uint32_t* select,
                            uint32_t* count, hipStream_t stream) {
    const uint64_t blocks = (n + kSelBlock - 1) / kSelBlock;
    if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
    if (blocks == 0) return hipMemsetAsync(count, 0, sizeof(uint32_t), stream);
    // the per-block counts: stream-ordered scratch, so calls on different streams never share it; a device
    // without memory pools gets a plain allocation, freed after the stream has drained
    int dev = 0, pools = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e == hipSuccess) e = hipDeviceGetAttribute(&pools, hipDeviceAttributeMemoryPoolsSupported, dev);
    if (e != hipSuccess) return e;
    uint32_t* counts = nullptr;
    e = pools ? hipMallocAsync(reinterpret_cast<void**>(&counts), blocks * sizeof(uint32_t), stream)
              : hipMalloc(reinterpret_cast<void**>(&counts), blocks * sizeof(uint32_t));
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(bf_select_count_kernel, dim3(static_cast<uint32_t>(blocks)), dim3(kSelBlock), 0, stream, scores,
                       bias, offsets, order, n, mu, lambda, threshold, pvalues, counts);
    e = hipGetLastError();
    if (e == hipSuccess) {
        hipLaunchKernelGGL(bf_select_scan_kernel, dim3(1), dim3(kScanBlock), 0, stream, counts,
                           static_cast<uint32_t>(blocks), count);
        e = hipGetLastError();
    }
    if (e == hipSuccess) {
        hipLaunchKernelGGL(bf_select_write_kernel, dim3(static_cast<uint32_t>(blocks)), dim3(kSelBlock), 0, stream,
                           scores, bias, offsets, order, n, mu, lambda, threshold, counts, select);
        e = hipGetLastError();
    }
    hipError_t f;
    if (pools) {
        f = hipFreeAsync(counts, stream);
    } else {
        f = hipStreamSynchronize(stream);
        const hipError_t g = hipFree(counts);
        if (f == hipSuccess) f = g;
    }
    return e != hipSuccess ? e : f;
}

__global__ __launch_bounds__(kSelBlock) void bf_pvalues_kernel(const float* __restrict__ scores,
                                                               const float* __restrict__ bias,
                                                               const uint64_t* __restrict__ offsets, uint64_t n,
                                                               float location, float scale, int kind,
                                                               double* __restrict__ pvalues) {
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kSelBlock + threadIdx.x;
    if (i >= n) return;
    const uint64_t L = offsets[i + 1] - offsets[i];
    pvalues[i] = kind == MSV_BF_GUMBEL ? msv_host::bf_gumbel_pvalue(scores[i], bias[i], L, location, scale)
                                       : msv_host::bf_exponential_pvalue(scores[i], bias[i], L, location, scale);
}

hipError_t launch_bf_pvalues(const float* scores, const float* bias, const uint64_t* offsets, uint64_t n,
                             float location, float scale, int kind, double* pvalues, hipStream_t stream) {
    const uint64_t blocks = (n + kSelBlock - 1) / kSelBlock;
    if (blocks == 0) return hipSuccess;
    if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(bf_pvalues_kernel, dim3(static_cast<uint32_t>(blocks)), dim3(kSelBlock), 0, stream, scores, bias,
                       offsets, n, location, scale, kind, pvalues);
    return hipGetLastError();
}

}  // namespace bfk
