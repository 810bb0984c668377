// spl_kernel.hip -- the split stage on gfx950: the recording Forward launch that keeps fM, fI and fD of
// every row of an envelope, and the stochastic traceback sampler over those planes.  msv.h states the model.
//
//   spl_fwd_kernel     one envelope per 64-lane wave, lane l holds the S consecutive states l*S+1 .. l*S+S, in
//                      aln_fwd_kernel's shape (its variant family, its table placement per S, the work queue of
//                      seq_queue.h): the Forward row of p7_forward_row.inc plus the stores.  After every row each
//                      lane stores its S values of fM, of fI and of fD (float bits, in the scale of the row's
//                      exponent) as [row][plane * S + slot][lane] -- a store instruction writes 256 contiguous
//                      bytes -- next to the six-word special-state record.  D is in registers when the row ends, so
//                      the third plane costs its stores only.  Plain vector stores only.
//   spl_sample_kernel  spl_host.h's spl_sample (the function the CPU definition runs), one (item, sample) per thread,
//                      the lanes of a wave consecutive samples of one item: a count pass, then a place pass with the
//                      same counters and so the same draws.  Only segments are written.
// An item whose envelope score is not finite is skipped by the sampler.
#include <hip/hip_runtime.h>

#include "msv_kernel.h"
#include "p7_rows.h"
#include "spl_host.h"
#include "spl_kernel.h"

namespace splk {

namespace {
__device__ __forceinline__ bool not_finite(uint32_t bits) { return (bits & 0x7f800000u) == 0x7f800000u; }
}  // namespace

// ------------------------------------------------------------------------------------------------
// The recording Forward kernel: the shared head, start and row (p7_rows.h), the record and the three planes.
// ------------------------------------------------------------------------------------------------
template <int S, bool ELDS, bool ISC, int WAVES>
__global__ __launch_bounds__(WAVES * 64) void spl_fwd_kernel(const SplArgs a) {
#include "p7_kernel_head.inc"
    while (item < total) {
        uint32_t s;
        uint64_t o0, L;
        if (seqq::take(a, item, lane, &s, &o0, &L)) {
            const uint32_t lc = __builtin_amdgcn_readfirstlane(a.lc[s]);
            const float2 lm = a.lentab[lc];
            const float loop = lm.x, move = lm.y;
#include "p7_forward_begin.inc"
            uint32_t* rec = a.ws + seqq::u64first(a.base[s]);
            float* mat = reinterpret_cast<float*>(rec + (L + 1) * kRowWords) + lane;  // row i at mat + i * 3 S 64
            auto record = [&](float E) {
                if (lane == 0) {
                    rec[0] = __float_as_uint(N);
                    rec[1] = __float_as_uint(J);
                    rec[2] = __float_as_uint(Cc);
                    rec[3] = __float_as_uint(B);
                    rec[4] = __float_as_uint(E);
                    rec[5] = static_cast<uint32_t>(e2);
                }
                rec += kRowWords;
            };
            record(0.0f);  // row 0
            const uint8_t* res = a.residues + o0;
            uint32_t cur = p7::residue_at(res, L, lane), nxt = p7::residue_at(res, L, 64 + lane);
            for (uint64_t i = 0; i < L; ++i) {
#include "p7_forward_row.inc"
                record(E);  // row i + 1, in the scale of its exponent
                // the row's fM, fI and fD, in that scale too: [plane * S + slot][lane], 256 contiguous bytes a store
                float* mrow = mat + i * (3 * S * kLanes);
#pragma unroll
                for (int q = 0; q < S; ++q) {
                    mrow[q * kLanes] = M[q];
                    mrow[(S + q) * kLanes] = I[q];
                    mrow[(2 * S + q) * kLanes] = D[q];
                }
            }
#include "p7_forward_end.inc"
        }
        item = seqq::next_item(a.counter, lane, nwaves);
    }
    seqq::last_exit<WAVES>(a.counter, &exited_s, lane);
}

// ------------------------------------------------------------------------------------------------
// The sampler, one (item, sample) per thread.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kSampleBlock) void spl_sample_kernel(const SampleArgs a) {
    using namespace msv_host;
    const uint32_t per_item = (a.n_samples + kSampleBlock - 1) / kSampleBlock;
    const uint32_t j = blockIdx.x / per_item;  // the item of the chunk
    const uint32_t sample = (blockIdx.x % per_item) * kSampleBlock + threadIdx.x;
    if (j >= a.hi - a.lo || sample >= a.n_samples) return;
    const uint32_t s = a.lo + j;
    const uint64_t at = static_cast<uint64_t>(j) * a.n_samples + sample;
    const uint64_t L = a.offsets[s + 1] - a.offsets[s];
    const bool write = a.segments != nullptr;
    uint32_t nd = 0;
    bool whole = true;
    if (L != 0 && !not_finite(__float_as_uint(a.scores[s]))) {
        const uint32_t S = a.S;
        const uint32_t* const rec0 = a.ws + a.base[s];
        const float* const mat = reinterpret_cast<const float*>(rec0 + spl_record_words(L));
        const msv_aln_item it = a.items[s];
        const SplOdds o{a.tr, a.tBM, a.tEC, a.tEJ, a.lentab[a.lc[s]].x};
        uint64_t seg_at = write ? a.seg_off[at + 1] : 0;
        const uint64_t seg_lo = write ? a.seg_off[at] : 0;
        whole = spl_sample(
            L, a.leng,
            [&](int p, uint64_t i, uint32_t k) -> float {
                const uint32_t v = (k - 1) / S, q = (k - 1) % S;
                return mat[((i - 1) * 3 * S + static_cast<uint32_t>(p) * S + q) * kLanes + v];
            },
            [&](uint64_t i, int w) -> uint32_t { return rec0[i * kRowWords + static_cast<uint32_t>(w)]; }, o,
            spl_key(a.seed, it.seq, it.i_from, it.i_to, sample), [](char, uint64_t, uint32_t) {},
            [&](uint32_t i_from, uint32_t i_to, uint32_t k_from, uint32_t k_to, uint32_t) {
                ++nd;
                if (write && seg_at > seg_lo) {  // (the count pass sized the span: never below its first entry)
                    msv_spl_segment g;
                    g.i_from = i_from + it.i_from - 1;
                    g.i_to = i_to + it.i_from - 1;
                    g.k_from = k_from;
                    g.k_to = k_to;
                    a.segments[--seg_at] = g;
                }
            });
    }
    if (!write) a.counts[at] = nd | (whole ? 0u : 0x80000000u);
}

// ------------------------------------------------------------------------------------------------
// Variant table: the alignment stage's family.
// ------------------------------------------------------------------------------------------------
#define SPL_VARIANT(S_, ELDS_, ISC_, W_, NAME_) \
    SplVariant{S_, ELDS_, ISC_, W_, reinterpret_cast<const void*>(&spl_fwd_kernel<S_, ELDS_, ISC_, W_>), NAME_}

const SplVariant* spl_variants(int* count) {
    static const SplVariant all[] = {
        SPL_VARIANT(2, true, false, 8, "spl_s2"),    SPL_VARIANT(6, true, false, 8, "spl_s6"),
        SPL_VARIANT(12, true, false, 8, "spl_s12"),  SPL_VARIANT(22, false, false, 8, "spl_s22g"),
        SPL_VARIANT(38, false, false, 4, "spl_s38g4"),
        SPL_VARIANT(2, true, true, 8, "spl_s2i"),    SPL_VARIANT(6, true, true, 8, "spl_s6i"),
        SPL_VARIANT(12, true, true, 8, "spl_s12i"),  SPL_VARIANT(22, false, true, 8, "spl_s22gi"),
        SPL_VARIANT(38, false, true, 4, "spl_s38g4i"),
    };
    *count = static_cast<int>(sizeof(all) / sizeof(all[0]));
    return all;
}

const void* sample_fn() { return reinterpret_cast<const void*>(&spl_sample_kernel); }

hipError_t spl_launch(const void* fn, int waves, uint32_t blocks, const SplArgs& args, hipStream_t stream) {
    void* params[] = {const_cast<SplArgs*>(&args)};
    return hipLaunchKernel(fn, dim3(blocks), dim3(waves * 64), params, 0, stream);
}

hipError_t launch_sample(const SampleArgs& a, hipStream_t stream) {
    if (a.hi <= a.lo || a.n_samples == 0) return hipSuccess;
    const uint64_t per_item = (a.n_samples + kSampleBlock - 1) / kSampleBlock;
    const uint64_t blocks = per_item * (a.hi - a.lo);
    if (blocks >= (1ull << 31)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(spl_sample_kernel, dim3(static_cast<uint32_t>(blocks)), dim3(kSampleBlock), 0, stream, a);
    return hipGetLastError();
}

}  // namespace splk
