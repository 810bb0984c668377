// aln_null2.hip -- the bias stage on gfx950 (msv.h "Bias stage"): the null2 model of each envelope "by
// expectation", from the posteriors Backward left in the alignment workspace (aln_host.h's layout, §4.11).
//
// The expectation is a column sum over the posterior matrix with no row-to-row dependency, so it is spread over rows
// as well as items.  Two launches per chunk, both read-only on the workspace:
//   aln_null2_partial<S>      a unit is (item, block of R = kNull2RowBlock consecutive rows); one wave a unit, lane l
//                             holding the S states l*S+1 .. l*S+S as every kernel of the stage.  The lane adds its
//                             [row][slot][lane] posteriors over the block's rows, ascending, into 2 S float32 sums (a
//                             load instruction covers 256 contiguous bytes; the rows are independent, so several
//                             rows' loads are in flight), and ppN + ppJ + ppC of the rows it strides.  The unit writes
//                             a slab of (2 S + 1) x 64 floats with plain vector stores.  No atomics.
//   aln_null2_finish<S, ISC>  one wave an item: adds the item's slabs in block order, forms per lane and residue x
//                             sum_slot eM etab[x] + eI itab[x] (slots beyond LENG and the insert slot of node LENG
//                             masked BY INDEX), sums across the lanes in wave_sum's fixed butterfly, adds the summed
//                             eX, multiplies by 1 / Le and writes null2[item][20].
// The float32 order of summation is a function of (S, Le, R) only: not of the chunk, the grid or the run.  An item
// whose envelope score is not finite is skipped by both (its null2 stays as the host set it: zeros).
#include <hip/hip_runtime.h>

#include "aln_host.h"
#include "aln_null2.h"
#include "null2_host.h"

namespace alnk {

namespace {

constexpr int kLanes = 64;
constexpr uint64_t kRowWords = msv_host::kAlnRowWords;
constexpr uint32_t R = static_cast<uint32_t>(msv_host::kNull2RowBlock);

__device__ __forceinline__ bool not_finite(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u; }

// every lane adds the same pairs in the same order (p7_rows.h's wave_sum), so all lanes hold the same bits
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// rows whose loads are issued together: 2 S loads a row
template <int S>
constexpr int rows_in_flight() {
    return S <= 6 ? 4 : S <= 12 ? 2 : 1;
}

}  // namespace

template <int S>
__global__ __launch_bounds__(kNull2Waves * 64) void aln_null2_partial(const Null2Args a) {
    constexpr int U = rows_in_flight<S>();
    const int lane = threadIdx.x & 63;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t u = blockIdx.x * kNull2Waves + wave;
    if (u >= a.units) return;
    const uint32_t s = __builtin_amdgcn_readfirstlane(a.unit_item[u]);
    if (s < a.lo || s >= a.hi || not_finite(a.scores[s])) return;
    const uint64_t L = a.offsets[s + 1] - a.offsets[s];
    const uint64_t i0 = static_cast<uint64_t>(u - a.unit_first[s]) * R;
    if (i0 >= L) return;
    const uint64_t i1 = i0 + R < L ? i0 + R : L;
    const uint32_t* const rec0 = a.ws + a.base[s];
    const float* const mat = reinterpret_cast<const float*>(rec0 + (L + 1) * kRowWords) + lane;

    float acc[2 * S];
#pragma unroll
    for (int q = 0; q < 2 * S; ++q) acc[q] = 0.0f;
    uint64_t i = i0;
    for (; i + U <= i1; i += U) {
        float v[U][2 * S];
#pragma unroll
        for (int r = 0; r < U; ++r) {
            const float* mrow = mat + (i + r) * (2 * S * kLanes);
#pragma unroll
            for (int q = 0; q < 2 * S; ++q) v[r][q] = mrow[q * kLanes];
        }
#pragma unroll
        for (int r = 0; r < U; ++r)
#pragma unroll
            for (int q = 0; q < 2 * S; ++q) acc[q] += v[r][q];
    }
    for (; i < i1; ++i) {
        const float* mrow = mat + i * (2 * S * kLanes);
#pragma unroll
        for (int q = 0; q < 2 * S; ++q) acc[q] += mrow[q * kLanes];
    }
    // residue i + 1 emitted by N, J or C: the first three words of row i + 1's record; lanes stride the rows
    float ex = 0.0f;
    for (uint64_t r = i0 + static_cast<uint64_t>(lane); r < i1; r += kLanes) {
        const uint32_t* const w = rec0 + (r + 1) * kRowWords;
        ex += (__uint_as_float(w[0]) + __uint_as_float(w[1])) + __uint_as_float(w[2]);
    }
    float* const slab = a.slabs + static_cast<uint64_t>(u) * msv_host::null2_slab_floats(S) + lane;
#pragma unroll
    for (int q = 0; q < 2 * S; ++q) slab[q * kLanes] = acc[q];
    slab[2 * S * kLanes] = ex;
}

template <int S, bool ISC>
__global__ __launch_bounds__(kNull2Waves * 64) void aln_null2_finish(const Null2Args a) {
    constexpr int C2 = S / 2;
    const int lane = threadIdx.x & 63;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t j = blockIdx.x * kNull2Waves + wave;
    if (j >= a.hi - a.lo) return;
    const uint32_t s = a.lo + j;
    if (not_finite(a.scores[s])) return;
    const uint64_t L = a.offsets[s + 1] - a.offsets[s];
    if (L == 0) return;
    const uint32_t nb = static_cast<uint32_t>((L + R - 1) / R);
    const uint32_t u0 = a.unit_first[s];
    if (u0 + nb > a.units) return;

    float eM[S], eI[S];
#pragma unroll
    for (int q = 0; q < S; ++q) eM[q] = eI[q] = 0.0f;
    float ex = 0.0f;
    for (uint32_t b = 0; b < nb; ++b) {
        const float* const slab = a.slabs + static_cast<uint64_t>(u0 + b) * msv_host::null2_slab_floats(S) + lane;
        // the slab's loads first, then its adds: a slab is one round trip, not 2 S + 1 (DESIGN 4.12 has the A/B)
        float v[2 * S + 1];
#pragma unroll
        for (int q = 0; q < 2 * S + 1; ++q) v[q] = slab[q * kLanes];
#pragma unroll
        for (int q = 0; q < S; ++q) {
            eM[q] += v[q];
            eI[q] += v[S + q];
        }
        ex += v[2 * S];
    }
    const float eX = wave_sum(ex);

    float mine = 0.0f;
#pragma unroll 2
    for (uint32_t x = 0; x < msv_host::kNull2Residues; ++x) {
        float t = 0.0f;
#pragma unroll
        for (int c = 0; c < C2; ++c) {
            const float2 e = a.etab[(x * C2 + c) * kLanes + lane];
            float2 in = make_float2(1.0f, 1.0f);
            if constexpr (ISC) in = a.itab[(x * C2 + c) * kLanes + lane];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int q = 2 * c + h;
                const uint32_t k = static_cast<uint32_t>(lane * S + q + 1);
                // masked by index: what the recording kernel leaves in padding slots, and the tables' padding, are
                // not relied on
                const float pm = eM[q] * (h ? e.y : e.x);
                const float pi = ISC ? eI[q] * (h ? in.y : in.x) : eI[q];
                t += k <= a.leng ? pm : 0.0f;
                t += k < a.leng ? pi : 0.0f;
            }
        }
        t = wave_sum(t);
        if (static_cast<uint32_t>(lane) == x) mine = t;
    }
    const float inv = 1.0f / static_cast<float>(L);
    if (static_cast<uint32_t>(lane) < msv_host::kNull2Residues)
        a.null2[static_cast<uint64_t>(s) * msv_host::kNull2Residues + lane] = (mine + eX) * inv;
}

#define NULL2_VARIANT(S_, ISC_)                                                             \
    Null2Variant{S_, ISC_, reinterpret_cast<const void*>(&aln_null2_partial<S_>),           \
                 reinterpret_cast<const void*>(&aln_null2_finish<S_, ISC_>)}

const Null2Variant* null2_variant(int S, bool isc) {
    static const Null2Variant all[] = {
        NULL2_VARIANT(2, false),  NULL2_VARIANT(6, false),  NULL2_VARIANT(12, false), NULL2_VARIANT(22, false),
        NULL2_VARIANT(38, false), NULL2_VARIANT(2, true),   NULL2_VARIANT(6, true),   NULL2_VARIANT(12, true),
        NULL2_VARIANT(22, true),  NULL2_VARIANT(38, true),
    };
    for (const Null2Variant& v : all)
        if (v.S == S && v.isc == isc) return &v;
    return nullptr;
}

namespace {
hipError_t launch(const void* fn, uint32_t waves, const Null2Args& a, hipStream_t stream) {
    if (waves == 0) return hipSuccess;
    void* params[] = {const_cast<Null2Args*>(&a)};
    return hipLaunchKernel(fn, dim3((waves + kNull2Waves - 1) / kNull2Waves), dim3(kNull2Waves * 64), params, 0, stream);
}
}  // namespace

hipError_t null2_launch_partial(const Null2Variant* v, const Null2Args& a, hipStream_t stream) {
    return launch(v->partial_fn, a.units, a, stream);
}
hipError_t null2_launch_finish(const Null2Variant* v, const Null2Args& a, hipStream_t stream) {
    return launch(v->finish_fn, a.hi - a.lo, a, stream);
}

}  // namespace alnk
