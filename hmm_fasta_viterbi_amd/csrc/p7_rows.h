// p7_rows.h -- the float32 Forward row and the mirrored Backward row of the one-sequence-per-wave stages, with the
// kernel frame around them, device side: fwd_kernel.hip, dom_kernel.hip (4.10) and aln_kernel.hip (4.11)
// are each "these rows plus the stage's own stores".  Every kernel computes a row in the same operation order, which
// is what holds the stages to one another's bits.  Device code only: no .cpp includes it.
//
// The shape: one sequence per 64-lane wave, lane l holds the S consecutive states l*S+1 .. l*S+S of M, I, D in
// VGPRs, wave-uniform residues in 64-row blocks, the slot arrays in LDS, the work queue of seq_queue.h.
//
// Two kinds of pieces, each written once.  Functions, here: the lane primitives, the residue fetch and the rescale
// decision, which compile into every kernel as the statements they replace did.  Text, in the .inc files beside this
// header, included inside the kernels (msv_kernel_body.inc's idiom): the statements that do NOT survive a function
// boundary unchanged -- as function templates the rows, the LDS staging, the slot accessor with its opaque zero, the
// residue reader, and in single variants even the table-row pointers and the score store, compiled to other
// instruction streams and register counts (work distribution, has the figures), and these kernels' code
// generation was paid for (no scratch at S = 22 and S = 38).  Each text names what it takes from the including scope.
//     p7_kernel_head.inc          a kernel's head: tables into LDS, scan multipliers, the accessor tlds, first item
//     p7_forward_begin.inc        what a sequence carries through Forward: M, I, D, N, J, C, B, the exponent
//     p7_forward_row.inc          the Forward row (fwd_kernel.hip states the recurrence); leaves E
//     p7_forward_end.inc          the Forward score and the bad-residue refusal
//     p7_backward_begin.inc       what a sequence carries through Backward, and its last residue blocks
//     p7_backward_specials.inc    the Backward row's first half (dom_kernel.hip states the recurrence)
//     p7_backward_cells.inc       its second half: the D chain, the mirrored scan, bM and bI in place
// (the two Backward halves name domk::B_*: their includers, dom_kernel.hip and aln_kernel.hip, have dom_kernel.h)
#pragma once

#include <hip/hip_runtime.h>

#include "fwd_kernel.h"
#include "msv_kernel.h"
#include "seq_queue.h"

namespace p7 {

using fwdk::kArrays;
using fwdk::kLanes;
using fwdk::kRows;
using fwdk::kScanSteps;

// ------------------------------------------------------------------------------------------------
// Lane primitives
// ------------------------------------------------------------------------------------------------
// Lane l-1's value into lane l, 0 into lane 0 (wave_shr:1), and lane l+1's value into lane l, 0 into lane 63
// (wave_shl:1): one DPP move across the wave each, bound_ctrl off (the lane without a source keeps `old`, which
// is 0).
constexpr int DPP_WAVE_SHR1 = 0x138;
constexpr int DPP_WAVE_SHL1 = 0x130;
__device__ __forceinline__ float shift1(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), DPP_WAVE_SHR1, 0xF, 0xF, false));
}
__device__ __forceinline__ float shift1_down(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), DPP_WAVE_SHL1, 0xF, 0xF, false));
}
// Lane l-d's value into lane l (d = 2 .. 32), 0 into lanes below d; lane l+d's value into lane l, 0 into lanes
// above 63-d: ds_bpermute_b32 (the LDS crossbar, no LDS memory) and a select.
__device__ __forceinline__ float shift_by(float v, int lane, int d) {
    const float t = __int_as_float(__builtin_amdgcn_ds_bpermute((lane - d) * 4, __float_as_int(v)));
    return lane >= d ? t : 0.0f;
}
__device__ __forceinline__ float shift_down_by(float v, int lane, int d) {
    const float t = __int_as_float(__builtin_amdgcn_ds_bpermute(((lane + d) & 63) * 4, __float_as_int(v)));
    return lane + d < kLanes ? t : 0.0f;
}
// The 64-lane sum as a butterfly: every lane adds the same pairs in the same order, so all lanes hold the same
// bits (a + b == b + a).
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// ------------------------------------------------------------------------------------------------
// The pieces of the rows that are functions (the rescale is three one-line values, not one function that decides:
// a helper that returns the exponent, 0 for none, compiled 50 of the 60 kernels differently)
// ------------------------------------------------------------------------------------------------
// The residues of a sequence reach the rows in 64-row blocks, lane l holding the block's residue l (the rows read
// them by v_readlane): the residue at index `at` of the L at `res`, 0 past the end.
template <class Index>
__device__ __forceinline__ uint32_t residue_at(const uint8_t* res, uint64_t L, Index at) {
    return static_cast<uint64_t>(at) < L ? res[at] : 0u;
}

// The rescaling of a row, decided on a wave-uniform sum E >= 0 (so its bits Eb order as floats, and the branch is
// scalar): when 2^32 < E < inf, everything the row carries is scaled down by 2^-x, x = E's exponent (at most 126,
// so 2^-x is a normal float): exact.  The exponents are summed per sequence and come back as e ln 2 in the score.
__device__ __forceinline__ bool past_2_32(uint32_t Eb) { return Eb > 0x4f800000u && Eb < 0x7f800000u; }
__device__ __forceinline__ uint32_t exponent_of(uint32_t Eb) {
    const uint32_t x = (Eb >> 23) - 127u;
    return x < 126u ? x : 126u;
}
__device__ __forceinline__ float pow2_minus(uint32_t x) { return __uint_as_float((127u - x) << 23); }

}  // namespace p7
