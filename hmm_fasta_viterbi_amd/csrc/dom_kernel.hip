// dom_kernel.hip -- the domain stage on gfx950: Backward, the per-residue domain posteriors that
// come from Forward x Backward on the special states, and the envelope rule.  msv.h states the model.
//
// Two persistent launches per chunk of selected sequences, both in fwd_kernel.hip's shape (one sequence per 64-lane
// wave, lane l holds the S consecutive states l*S+1 .. l*S+S, wave-uniform residues in 64-row blocks, the work
// queue of seq_queue.h) and with its table placement per S:
//   dom_fwd_kernel  Forward's row -- p7_forward_row.inc, the text fwd_kernel includes --; after every row lane 0 stores
//                   the row's N, J, C, B, E and the running exponent -- six words, row 0 included -- to the workspace.
//                   The arithmetic and its order are fwd_kernel's, so the final score has its bits.
//   dom_bck_kernel  rows L down to 0.  In odds, with P(k) = m[r][k] bM'(k), H(k) = ins[r][k] bI'(k) (' = row i+1):
//                       bB = tBM sum_k P(k);  bJ = loop bJ' + move bB;  bC = loop bC';  bN = loop bN' + move bB;
//                       bE = tEJ bJ + tEC bC
//                       bD(k) = [k>=2] bE + tDM[k] P(k+1) + tDD[k] bD(k+1)       <- within the row, right to left
//                       bM(k) = bE + tMM[k] P(k+1) + tMI[k] H(k) + tMD[k] bD(k+1)
//                       bI(k) = tIM[k] P(k+1) + tII[k] H(k)
//                   The D chain is Forward's three-phase scan mirrored: every lane runs its slots from the TOP with
//                   an incoming 0 (the exits bE enter every D with k >= 2, so a lane's constant term is its whole
//                   local chain, not one transition), an inclusive scan of the lanes' affine maps towards lane 0
//                   (6 steps, suffix products of tDD precomputed on the host), one FMA per slot with the slot's
//                   suffix product.  P(k+1) of a lane's last slot and the D entering a lane come from the lane on
//                   the right by one DPP wave_shl:1.  sum_k P is the row's one wave reduction; the rescaling (an
//                   exact power of two, its own running exponent) is decided on it, before tBM is applied.
//                   Per row lane 0 reads the row's Forward record and writes end[i], begin[i+1] and occ[i+1].
//   dom_regions_*   the envelope rule (dom_host.h's dom_regions_scan, the same function the CPU runs), one sequence
//                   per thread: count, an exclusive scan, place.
#include <hip/hip_runtime.h>

#include "dom_host.h"
#include "dom_kernel.h"
#include "msv_kernel.h"
#include "p7_rows.h"

namespace domk {

namespace {

// The first workspace row of list entry `item` (sequence s, first residue o0)
__device__ __forceinline__ uint64_t first_row(const DomArgs& a, uint32_t item, uint32_t s, uint64_t o0) {
    return a.item_rows ? seqq::u64first(a.item_rows[item]) : o0 + s;
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// The recording Forward kernel: the shared head, start and row (p7_rows.h) plus the record stores.
// ------------------------------------------------------------------------------------------------
template <int S, bool ELDS, bool ISC, int WAVES>
__global__ __launch_bounds__(WAVES * 64) void dom_fwd_kernel(const DomArgs a) {
#include "p7_kernel_head.inc"
    while (item < total) {
        uint32_t s;
        uint64_t o0, L;
        if (seqq::take(a, item, lane, &s, &o0, &L)) {
            const float2 lm = a.lentab[L];
            const float loop = lm.x, move = lm.y;
#include "p7_forward_begin.inc"
            // the sequence's records: row i at rec + i * kRowWords (null: nothing is recorded)
            uint32_t* rec = a.records ? a.records + first_row(a, item, s, o0) * kRowWords : nullptr;
            auto record = [&](float E) {
                if (rec && lane == 0) {
                    rec[0] = __float_as_uint(N);
                    rec[1] = __float_as_uint(J);
                    rec[2] = __float_as_uint(Cc);
                    rec[3] = __float_as_uint(B);
                    rec[4] = __float_as_uint(E);
                    rec[5] = static_cast<uint32_t>(e2);
                }
                if (rec) rec += kRowWords;
            };
            record(0.0f);  // row 0
            // the first two residue blocks: `cur` is the block of the row, `nxt` the one after it
            const uint8_t* res = a.residues + o0;
            uint32_t cur = p7::residue_at(res, L, lane), nxt = p7::residue_at(res, L, 64 + lane);
            for (uint64_t i = 0; i < L; ++i) {
#include "p7_forward_row.inc"
                record(E);  // row i + 1, in the scale of its exponent
            }
#include "p7_forward_end.inc"
        }
        item = seqq::next_item(a.counter, lane, nwaves);
    }
    seqq::last_exit<WAVES>(a.counter, &exited_s, lane);
}

// ------------------------------------------------------------------------------------------------
// Backward with the posteriors: the shared head, start and row halves (p7_rows.h), the posteriors between the halves.
// ------------------------------------------------------------------------------------------------
template <int S, bool ELDS, bool ISC, int WAVES>
__global__ __launch_bounds__(WAVES * 64) void dom_bck_kernel(const DomArgs a) {
#include "p7_kernel_head.inc"
    while (item < total) {
        uint32_t s;
        uint64_t o0, L;
        // (take refuses as the recording launch did: -inf for an empty sequence, NaN for one too long)
        if (seqq::take(a, item, lane, &s, &o0, &L)) {
            const uint32_t fwd_bits = __builtin_amdgcn_readfirstlane(__float_as_uint(a.fwd_scores[s]));
            if ((fwd_bits & 0x7f800000u) == 0x7f800000u) {
                // the recording launch refused the sequence (a bad residue: +inf): its class, no posteriors
                if (lane == 0) a.scores[s] = __uint_as_float(fwd_bits);
            } else {
                const float2 lm = a.lentab[L];
                const float loop = lm.x, move = lm.y;
                const uint32_t* const rec0 = a.records + first_row(a, item, s, o0) * kRowWords;
                // Z = fC(L) move 2^efL
                // (its reciprocal, taken once in float64: the rows multiply, 2^-53 beside the factors' 2^-24)
                const double invZ = 1.0 / static_cast<double>(__uint_as_float(rec0[L * kRowWords + 2]) * move);
                const int32_t efL = static_cast<int32_t>(rec0[L * kRowWords + 5]);
#include "p7_backward_begin.inc"
                float bNout = 0.0f;
                for (uint64_t i = L + 1; i-- > 0;) {
                    // this row's Forward record, asked for before the row's first pass
                    const uint32_t* const r6 = rec0 + i * kRowWords;
                    const float fN = __uint_as_float(r6[0]), fJ = __uint_as_float(r6[1]), fC = __uint_as_float(r6[2]);
                    const float fB = __uint_as_float(r6[3]), fE = __uint_as_float(r6[4]);
                    const int32_t ef = static_cast<int32_t>(r6[5]);
#include "p7_backward_specials.inc"
                    bNout = bN;

                    // the posteriors this row completes -- end[i], begin[i+1], occ[i+1] -- need the specials only
                    // and stand here, before the passes over the slots: behind them, the compiler sinks the last
                    // pass below this branch and keeps its table values live across it (S = 22 spilled).  The two
                    // scales combine by an exact ldexp; float64 products, so no range is lost (one lane, a handful
                    // of operations)
                    if (lane == 0) {
                        const int sh = ef + e2 - efL;
                        if (i >= 1)
                            a.end[o0 + i - 1] = static_cast<float>(
                                ldexp(static_cast<double>(fE) * static_cast<double>(bE) * invZ, sh));
                        if (i < L) {
                            a.begin[o0 + i] = static_cast<float>(
                                ldexp(static_cast<double>(fB) * static_cast<double>(bB) * invZ, sh));
                            const double out = static_cast<double>(fN) * static_cast<double>(lN) +
                                               static_cast<double>(fJ) * static_cast<double>(lJ) +
                                               static_cast<double>(fC) * static_cast<double>(lC);
                            a.occ[o0 + i] = static_cast<float>(1.0 - ldexp(out * invZ, sh));
                        }
                    }

#include "p7_backward_cells.inc"
                }
                const float sc = fmaf(static_cast<float>(e2), 0.69314718055994529f, logf(bNout));
                if (lane == 0) a.scores[s] = sc;
            }
        }
        item = seqq::next_item(a.counter, lane, nwaves);
    }
    seqq::last_exit<WAVES>(a.counter, &exited_s, lane);
}

// ------------------------------------------------------------------------------------------------
// The envelope rule, one list entry per thread.
// ------------------------------------------------------------------------------------------------
namespace {

constexpr int kRegBlock = 64;
constexpr int kScanBlock = 256;

// The sequence of list entry q and whether the rule runs on it (its Forward score finite, so its arrays written)
__device__ __forceinline__ bool region_entry(const RegionArgs& a, uint64_t q, uint32_t* s, uint64_t* o0, uint64_t* L) {
    *s = a.select ? a.select[q] : static_cast<uint32_t>(q);
    if (*s >= a.n) return false;
    *o0 = a.offsets[*s];
    *L = a.offsets[*s + 1] - *o0;
    const uint32_t bits = __float_as_uint(a.fwd_scores[*s]);
    return *L > 0 && (bits & 0x7f800000u) != 0x7f800000u;
}

}  // namespace

__global__ __launch_bounds__(kRegBlock) void dom_regions_count(const RegionArgs a, uint32_t* __restrict__ counts) {
    const uint64_t q = static_cast<uint64_t>(blockIdx.x) * kRegBlock + threadIdx.x;
    if (q >= a.m) return;
    uint32_t s, c = 0;
    uint64_t o0, L;
    if (region_entry(a, q, &s, &o0, &L))
        c = msv_host::dom_regions_scan(a.begin + o0, a.end + o0, a.occ + o0, L, a.rt1, a.rt2,
                                       [](uint32_t, uint32_t, float, float) {});
    counts[q] = c;
}

// region_offsets[0 .. m]: the exclusive scan of counts, by one workgroup (each thread a contiguous strip)
__global__ __launch_bounds__(kScanBlock) void dom_regions_offsets(const uint32_t* __restrict__ counts, uint64_t m,
                                                                  uint64_t* __restrict__ region_offsets) {
    __shared__ uint64_t part[kScanBlock];
    const uint64_t strip = (m + kScanBlock - 1) / kScanBlock;
    const uint64_t lo = static_cast<uint64_t>(threadIdx.x) * strip < m ? static_cast<uint64_t>(threadIdx.x) * strip : m;
    const uint64_t hi = lo + strip < m ? lo + strip : m;
    uint64_t sum = 0;
    for (uint64_t q = lo; q < hi; ++q) sum += counts[q];
    part[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t run = 0;
        for (int t = 0; t < kScanBlock; ++t) {
            const uint64_t v = part[t];
            part[t] = run;
            run += v;
        }
        region_offsets[m] = run;
    }
    __syncthreads();
    uint64_t run = part[threadIdx.x];
    for (uint64_t q = lo; q < hi; ++q) {
        region_offsets[q] = run;
        run += counts[q];
    }
}

__global__ __launch_bounds__(kRegBlock) void dom_regions_place(const RegionArgs a,
                                                               const uint64_t* __restrict__ region_offsets,
                                                               msv_dom_region* __restrict__ regions) {
    const uint64_t q = static_cast<uint64_t>(blockIdx.x) * kRegBlock + threadIdx.x;
    if (q >= a.m) return;
    uint32_t s;
    uint64_t o0, L;
    if (!region_entry(a, q, &s, &o0, &L)) return;
    msv_dom_region* out = regions + region_offsets[q];
    msv_host::dom_regions_scan(a.begin + o0, a.end + o0, a.occ + o0, L, a.rt1, a.rt2,
                               [&](uint32_t i_from, uint32_t i_to, float nd, float mass) {
                                   *out++ = msv_dom_region{s, i_from, i_to, nd, mass};
                               });
}

namespace {
hipError_t region_grid(uint64_t m, uint32_t* blocks) {
    const uint64_t b = (m + kRegBlock - 1) / kRegBlock;
    if (b > 0x7fffffffull) return hipErrorInvalidValue;
    *blocks = static_cast<uint32_t>(b);
    return hipSuccess;
}
}  // namespace

hipError_t launch_regions_count(const RegionArgs& a, uint32_t* counts, hipStream_t stream) {
    uint32_t blocks = 0;
    const hipError_t e = region_grid(a.m, &blocks);
    if (e != hipSuccess || blocks == 0) return e;
    hipLaunchKernelGGL(dom_regions_count, dim3(blocks), dim3(kRegBlock), 0, stream, a, counts);
    return hipGetLastError();
}

hipError_t launch_regions_scan(const uint32_t* counts, uint64_t m, uint64_t* region_offsets, hipStream_t stream) {
    hipLaunchKernelGGL(dom_regions_offsets, dim3(1), dim3(kScanBlock), 0, stream, counts, m, region_offsets);
    return hipGetLastError();
}

hipError_t launch_regions_place(const RegionArgs& a, const uint64_t* region_offsets, msv_dom_region* regions,
                                hipStream_t stream) {
    uint32_t blocks = 0;
    const hipError_t e = region_grid(a.m, &blocks);
    if (e != hipSuccess || blocks == 0) return e;
    hipLaunchKernelGGL(dom_regions_place, dim3(blocks), dim3(kRegBlock), 0, stream, a, region_offsets, regions);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// Variant table: Forward's family and placement (fwd_kernel.hip), one pair of kernels per S and insert mode.
// ------------------------------------------------------------------------------------------------
#define DOM_VARIANT(S_, ELDS_, ISC_, W_, NAME_)                                                    \
    DomVariant{S_, ELDS_, ISC_, W_, reinterpret_cast<const void*>(&dom_fwd_kernel<S_, ELDS_, ISC_, W_>), \
               reinterpret_cast<const void*>(&dom_bck_kernel<S_, ELDS_, ISC_, W_>), NAME_}

const DomVariant* dom_variants(int* count) {
    static const DomVariant all[] = {
        DOM_VARIANT(2, true, false, 8, "dom_s2"),    DOM_VARIANT(6, true, false, 8, "dom_s6"),
        DOM_VARIANT(12, true, false, 8, "dom_s12"),  DOM_VARIANT(22, false, false, 8, "dom_s22g"),
        DOM_VARIANT(38, false, false, 4, "dom_s38g4"),
        DOM_VARIANT(2, true, true, 8, "dom_s2i"),    DOM_VARIANT(6, true, true, 8, "dom_s6i"),
        DOM_VARIANT(12, true, true, 8, "dom_s12i"),  DOM_VARIANT(22, false, true, 8, "dom_s22gi"),
        DOM_VARIANT(38, false, true, 4, "dom_s38g4i"),
    };
    *count = static_cast<int>(sizeof(all) / sizeof(all[0]));
    return all;
}

hipError_t dom_launch(const void* fn, int waves, uint32_t blocks, const DomArgs& args, hipStream_t stream) {
    void* params[] = {const_cast<DomArgs*>(&args)};
    return hipLaunchKernel(fn, dim3(blocks), dim3(waves * 64), params, 0, stream);
}

}  // namespace domk
