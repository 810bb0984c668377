// fwd_kernel.hip -- the Forward stage as ONE persistent gfx950 kernel per batch: the log of the summed
// odds of EVERY alignment of a sequence to the profile, the score HMMER3's E-values come from.
//
// msv.h states the model (the Viterbi stage's paths plus the D_k -> E exits of p7_GForward).  In odds x = exp(score),
// row i, residue r, k = 1..LENG:
//     M(i,k) = m[r][k] * (M'(k-1) tMM + I'(k-1) tIM + D'(k-1) tDM + B' tBM)
//     I(i,k) = ins[r][k] * (M'(k) tMI + I'(k) tII)
//     D(i,k) = M(i,k-1) tMD + D(i,k-1) tDD                     <- within the row: a linear recurrence
//     E = sum_k M(i,k) + D(i,k);  N *= loop;  J = J loop + E tEJ;  C = C loop + E tEC;  B = (N + J) move
//
// The shape is vit_kernel.hip's (one sequence per 64-lane wave, lane l holds the S consecutive states
// l*S+1 .. l*S+S of M, I, D in VGPRs, wave-uniform residues in 64-row blocks) on the same work queue
// (seq_queue.h: persistent grid, select / select_count, error bits).  What differs:
//   * float32 odds, rescaled by an exact power of two whenever the row's E passes 2^32 (E is wave-uniform, so the
//     branch is scalar); the exponent is summed per sequence and comes back as e ln 2 in the score;
//   * the D chain across lanes is a scan, not a lazy-F fix-point: every lane runs its S slots from an incoming 0,
//     one inclusive scan of the lanes' affine maps D_out = a D_in + b follows (6 steps, their multipliers
//     sequence-independent products of tDD, precomputed on the host), then one FMA per slot D_q += D_in c_q;
//   * E, J, C and B are sums, taken on every row: one 64-lane sum of the lanes' E, then scalar J, C, N, B;
//     B' tBM is the last term added in the M update, so the next row's other terms do not wait for it.
// A sequence is computed by one wave in a fixed operation order, so its score does not depend on its place in
// the batch, on the select list or on the stream.  Variants differ in S, that is in the order of summation, so
// their scores may differ in the last bits.
// The row and the kernel's frame are written once, in p7_rows.h and the text it documents (p7_kernel_head.inc,
// p7_forward_begin.inc, p7_forward_row.inc, p7_forward_end.inc): the domain and the alignment stage record this
// very row.
#include <hip/hip_runtime.h>

#include "fwd_host.h"
#include "fwd_kernel.h"
#include "msv_kernel.h"
#include "p7_rows.h"

namespace fwdk {

// Nothing is this kernel's own but the order of the shared pieces: the recording kernels add their stores to it.
template <int S, bool ELDS, bool ISC, int WAVES>
__global__ __launch_bounds__(WAVES * 64) void fwd_kernel(const FwdArgs a) {
#include "p7_kernel_head.inc"
    while (item < total) {
        uint32_t s;
        uint64_t o0, L;
        if (seqq::take(a, item, lane, &s, &o0, &L)) {
            const float2 lm = a.lentab[L];
            const float loop = lm.x, move = lm.y;
#include "p7_forward_begin.inc"
            // the first two residue blocks: `cur` is the block of the row, `nxt` the one after it
            const uint8_t* res = a.residues + o0;
            uint32_t cur = p7::residue_at(res, L, lane), nxt = p7::residue_at(res, L, 64 + lane);
            for (uint64_t i = 0; i < L; ++i) {
#include "p7_forward_row.inc"
            }
#include "p7_forward_end.inc"
        }
        item = seqq::next_item(a.counter, lane, nwaves);
    }
    seqq::last_exit<WAVES>(a.counter, &exited_s, lane);
}

namespace {
constexpr int kPvBlock = 256;
}

__global__ __launch_bounds__(kPvBlock) void fwd_pvalues_kernel(const float* __restrict__ scores,
                                                               const uint64_t* __restrict__ offsets, uint64_t n,
                                                               float tau, float lambda, double* __restrict__ pvalues) {
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kPvBlock + threadIdx.x;
    if (i < n) pvalues[i] = msv_host::fwd_pvalue_of(scores[i], offsets[i + 1] - offsets[i], tau, lambda);
}

hipError_t launch_fwd_pvalues(const float* scores, const uint64_t* offsets, uint64_t n, float tau, float lambda,
                              double* pvalues, hipStream_t stream) {
    const uint64_t blocks = (n + kPvBlock - 1) / kPvBlock;
    if (blocks == 0) return hipSuccess;
    if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(fwd_pvalues_kernel, dim3(static_cast<uint32_t>(blocks)), dim3(kPvBlock), 0, stream, scores,
                       offsets, n, tau, lambda, pvalues);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// Variant table: one per S and insert mode.  The 8 slot arrays are always in LDS (re-read every row); the match
// odds are in LDS up to S = 12 (61 KB + 25 KB) and read from L2 beyond (at S = 22 they would take 112 KB on top
// of 45 KB of slot arrays: one workgroup per CU with nothing to spare); insert odds come from L2.  S = 38 runs
// one wave per SIMD (4 per workgroup) for the 512-register budget.  DESIGN 4.9 records the placement per S.
// ------------------------------------------------------------------------------------------------
#define FWD_VARIANT(S_, ELDS_, ISC_, W_, NAME_) \
    FwdVariant{S_, ELDS_, ISC_, W_, reinterpret_cast<const void*>(&fwd_kernel<S_, ELDS_, ISC_, W_>), NAME_}

const FwdVariant* fwd_variants(int* count) {
    static const FwdVariant all[] = {
        FWD_VARIANT(2, true, false, 8, "fwd_s2"),    FWD_VARIANT(6, true, false, 8, "fwd_s6"),
        FWD_VARIANT(12, true, false, 8, "fwd_s12"),  FWD_VARIANT(22, false, false, 8, "fwd_s22g"),
        FWD_VARIANT(38, false, false, 4, "fwd_s38g4"),
        FWD_VARIANT(2, true, true, 8, "fwd_s2i"),    FWD_VARIANT(6, true, true, 8, "fwd_s6i"),
        FWD_VARIANT(12, true, true, 8, "fwd_s12i"),  FWD_VARIANT(22, false, true, 8, "fwd_s22gi"),
        FWD_VARIANT(38, false, true, 4, "fwd_s38g4i"),
    };
    *count = static_cast<int>(sizeof(all) / sizeof(all[0]));
    return all;
}

hipError_t fwd_launch(const FwdVariant& v, uint32_t blocks, const FwdArgs& args, hipStream_t stream) {
    void* params[] = {const_cast<FwdArgs*>(&args)};
    return hipLaunchKernel(v.fn, dim3(blocks), dim3(v.waves * 64), params, 0, stream);
}

}  // namespace fwdk
