// aln_kernel.hip -- the alignment stage on gfx950: posterior decoding of every (residue, state) cell
// of an envelope, the optimal-accuracy (OA) alignment over those posteriors, and its trace.  msv.h states the model.
//
// One envelope per 64-lane wave, lane l holds the S consecutive states l*S+1 .. l*S+S, in dom_kernel.hip's shape
// (its variant family, its table placement per S, the work queue of seq_queue.h).  Four launch kinds per chunk:
//   aln_fwd_kernel   the Forward row of p7_forward_row.inc (fwd_kernel's and dom_fwd_kernel's) plus the stores: after
//                    every row each lane stores its S values of fM and of fI (float bits, in the scale of the row's
//                    exponent) as [row][slot][lane] -- a store instruction writes 256 contiguous bytes -- next to the
//                    six-word special-state record.  loop / move are those of the item's CONFIGURED length lc[s].
//   aln_bck_kernel   the Backward row of p7_backward_*.inc (dom_bck_kernel's); once bM and bI of row i stand, the
//                    lane loads the row's fM and fI and writes ppM and ppI over them:
//                    (float) ldexp((double) f * (double) b * invZ, ef(i) + eb - ef(Le)).
//                    The product of two floats is exact in float64, the ldexp is applied to the product (whose
//                    true value is <= 1), so no pair of exponents loses range.  Lane 0 writes ppN, ppJ, ppC of
//                    residue i + 1 over the first three words of row i + 1's record, which Backward has read.
//   aln_fill_kernel  the max-plus OA row over the stored posteriors.  M comes from the previous row shifted by one
//                    state (the wave_shr:1 DPP move Forward uses); D, which adds nothing, is a gated running max: an
//                    in-lane pass from -inf, then a 6-step cross-lane scan of (is the lane's d->d chain open end to
//                    end -- constant over rows, so scanned once per item --, the lane's outgoing value), then one
//                    max per slot with the lane's incoming value where the chain from the lane's edge is open.  max
//                    is exact, so every D has the serial chain's bits.  4-bit back-pointers per cell and one record
//                    word per row in vit_trace_plan.h's encoding, found by equality on final values in msv.h's
//                    tie-break order.  Plain vector stores only.
//   aln_walk_kernel  aln_host.h's aln_walk (the function the CPU definition runs), one item per thread: a count
//                    pass, then a place pass that also gathers each op's posterior.
// An item whose envelope score is not finite is skipped by the last three.
#include <hip/hip_runtime.h>

#include "aln_host.h"
#include "aln_kernel.h"
#include "msv_kernel.h"
#include "p7_rows.h"
#include "vit_trace_plan.h"

namespace alnk {

namespace {

constexpr float NINF = -__builtin_inff();

using p7::shift1;  // (the fill shifts M, I, D by one state as Forward does)

__device__ __forceinline__ float wave_max(float x) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) x = fmaxf(x, __shfl_xor(x, d, 64));
    return x;
}
__device__ __forceinline__ uint32_t wave_min(uint32_t x) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t y = static_cast<uint32_t>(__shfl_xor(static_cast<int>(x), d, 64));
        x = y < x ? y : x;
    }
    return x;
}
__device__ __forceinline__ bool not_finite(uint32_t bits) { return (bits & 0x7f800000u) == 0x7f800000u; }

}  // namespace

// ------------------------------------------------------------------------------------------------
// The recording Forward kernel: the shared head, start and row (p7_rows.h), the record and the matrix stores.
// ------------------------------------------------------------------------------------------------
template <int S, bool ELDS, bool ISC, int WAVES>
__global__ __launch_bounds__(WAVES * 64) void aln_fwd_kernel(const AlnArgs a) {
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
            float* mat = reinterpret_cast<float*>(rec + (L + 1) * kRowWords) + lane;  // row i at mat + i * 2 S 64
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
            // the first two residue blocks: `cur` is the block of the row, `nxt` the one after it
            const uint8_t* res = a.residues + o0;
            uint32_t cur = p7::residue_at(res, L, lane), nxt = p7::residue_at(res, L, 64 + lane);
            for (uint64_t i = 0; i < L; ++i) {
#include "p7_forward_row.inc"
                record(E);  // row i + 1, in the scale of its exponent
                // the row's fM and fI, in that scale too: [slot][lane], 256 contiguous bytes a store
                float* mrow = mat + i * (2 * S * kLanes);
#pragma unroll
                for (int q = 0; q < S; ++q) {
                    mrow[q * kLanes] = M[q];
                    mrow[(S + q) * kLanes] = I[q];
                }
            }
#include "p7_forward_end.inc"
        }
        item = seqq::next_item(a.counter, lane, nwaves);
    }
    seqq::last_exit<WAVES>(a.counter, &exited_s, lane);
}

// ------------------------------------------------------------------------------------------------
// Backward with the per-cell combine.
// ------------------------------------------------------------------------------------------------
template <int S, bool ELDS, bool ISC, int WAVES>
__global__ __launch_bounds__(WAVES * 64) void aln_bck_kernel(const AlnArgs a) {
#include "p7_kernel_head.inc"
    while (item < total) {
        const uint32_t s = __builtin_amdgcn_readfirstlane(a.select[item]);
        const uint32_t fwd_bits = s < a.n ? __builtin_amdgcn_readfirstlane(__float_as_uint(a.scores[s])) : 0x7fc00000u;
        // (an item the recording launch refused -- a bad residue: +inf -- has no posteriors)
        if (!not_finite(fwd_bits)) {
            const uint64_t o0 = seqq::u64first(a.offsets[s]);
            const uint64_t L = seqq::u64first(a.offsets[s + 1]) - o0;
            const uint32_t lc = __builtin_amdgcn_readfirstlane(a.lc[s]);
            const float2 lm = a.lentab[lc];
            const float loop = lm.x, move = lm.y;
            uint32_t* const rec0 = a.ws + seqq::u64first(a.base[s]);
            float* const mat = reinterpret_cast<float*>(rec0 + (L + 1) * kRowWords) + lane;
            // Z = fC(L) move 2^efL, its reciprocal taken once in float64
            const double invZ = 1.0 / static_cast<double>(__uint_as_float(rec0[L * kRowWords + 2]) * move);
            const int32_t efL = static_cast<int32_t>(rec0[L * kRowWords + 5]);
#include "p7_backward_begin.inc"
            for (uint64_t i = L + 1; i-- > 0;) {
                const uint32_t* const r6 = rec0 + i * kRowWords;
                const float fN = __uint_as_float(r6[0]), fJ = __uint_as_float(r6[1]), fC = __uint_as_float(r6[2]);
                const int32_t ef = static_cast<int32_t>(r6[5]);
#include "p7_backward_specials.inc"

                // residue i + 1 emitted by N, J or C: over the first three words of row i + 1's record, which the
                // previous iteration read (before the passes over the slots, as dom_bck_kernel places its own)
                const int sh = ef + e2 - efL;
                if (lane == 0 && i < L) {
                    uint32_t* const w = rec0 + (i + 1) * kRowWords;
                    w[0] = __float_as_uint(static_cast<float>(
                        ldexp(static_cast<double>(fN) * static_cast<double>(lN) * invZ, sh)));
                    w[1] = __float_as_uint(static_cast<float>(
                        ldexp(static_cast<double>(fJ) * static_cast<double>(lJ) * invZ, sh)));
                    w[2] = __float_as_uint(static_cast<float>(
                        ldexp(static_cast<double>(fC) * static_cast<double>(lC) * invZ, sh)));
                }

#include "p7_backward_cells.inc"
                // the combine: row i's fM, fI become ppM, ppI in place, two slots at a time
                if (i >= 1) {
                    float* mrow = mat + (i - 1) * (2 * S * kLanes);
#pragma unroll
                    for (int c = 0; c < C2; ++c) {
#pragma unroll
                        for (int h = 0; h < 2; ++h) {
                            const int q = 2 * c + h;
                            const double pm = static_cast<double>(mrow[q * kLanes]) * static_cast<double>(M[q]) * invZ;
                            const double pi =
                                static_cast<double>(mrow[(S + q) * kLanes]) * static_cast<double>(I[q]) * invZ;
                            mrow[q * kLanes] = static_cast<float>(ldexp(pm, sh));
                            mrow[(S + q) * kLanes] = static_cast<float>(ldexp(pi, sh));
                        }
                        if constexpr (FENCE) __builtin_amdgcn_sched_barrier(0);
                    }
                }
            }
        }
        item = seqq::next_item(a.counter, lane, nwaves);
    }
    seqq::last_exit<WAVES>(a.counter, &exited_s, lane);
}

// ------------------------------------------------------------------------------------------------
// The OA fill: a max-plus row over the stored posteriors, 4 source bits per cell.
// ------------------------------------------------------------------------------------------------
template <int S>
__global__ __launch_bounds__(kFillWaves * 64) void aln_fill_kernel(const AlnArgs a) {
    using namespace vittrace;
    using namespace msv_host;
    constexpr int W = (S + kCellsPerWord - 1) / kCellsPerWord;
    constexpr int GW = (S + 3) / 4;
    __shared__ uint32_t exited_s;
    const int lane = threadIdx.x & 63;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t total = seqq::list_total(a);
    if (seqq::no_item<kFillWaves>(total)) {
        if (threadIdx.x == 0) seqq::count_leavers<1, 1>(a.counter);
        return;
    }
    if (threadIdx.x == 0) exited_s = 0;
    __syncthreads();

    uint32_t G[GW];
#pragma unroll
    for (int w = 0; w < GW; ++w) G[w] = a.gates[w * kLanes + lane];
    auto gate = [&](int q) -> uint32_t { return G[q >> 2] >> ((q & 3) * 8); };
    // the d->d chain's scan flags, constant over rows: bit j = "at step j this lane takes the value 2^j lanes to
    // its left", i.e. the lanes gathered so far are open end to end
    uint32_t chain = 1u;
#pragma unroll
    for (int q = 0; q < S; ++q) chain &= (gate(q) & kGateDD) ? 1u : 0u;
    uint32_t steps = 0;
#pragma unroll
    for (int j = 0; j < kScanSteps; ++j) {
        const int d = 1 << j;
        const uint32_t left = static_cast<uint32_t>(__shfl_up(static_cast<int>(chain), d, 64));
        if (lane >= d) {
            steps |= chain << j;
            chain &= left;
        }
    }

    const uint32_t nwaves = gridDim.x * kFillWaves;
    uint32_t item = blockIdx.x * kFillWaves + wave;
    while (item < total) {
        const uint32_t s = __builtin_amdgcn_readfirstlane(a.select[item]);
        const uint32_t fwd_bits = s < a.n ? __builtin_amdgcn_readfirstlane(__float_as_uint(a.scores[s])) : 0x7fc00000u;
        if (!not_finite(fwd_bits)) {
            const uint64_t o0 = seqq::u64first(a.offsets[s]);
            const uint64_t L = seqq::u64first(a.offsets[s + 1]) - o0;
            const uint32_t lc = __builtin_amdgcn_readfirstlane(a.lc[s]);
            const bool open_move = a.lentab[lc].y > 0.0f;
            const uint32_t* const rec0 = a.ws + seqq::u64first(a.base[s]);
            const float* const mat = reinterpret_cast<const float*>(rec0 + (L + 1) * kRowWords) + lane;
            uint32_t* const ptrs = a.ws + seqq::u64first(a.base[s]) + aln_record_words(L) + aln_matrix_words(S, L);
            uint32_t* const recs = ptrs + L * (static_cast<uint64_t>(W) * kLanes);
            float M[S], I[S], D[S];
#pragma unroll
            for (int q = 0; q < S; ++q) M[q] = I[q] = D[q] = NINF;
            float J = NINF, C = NINF, N = 0.0f, B = open_move ? 0.0f : NINF;
            for (uint64_t i = 0; i < L; ++i) {
                const float* mrow = mat + i * (2 * S * kLanes);
                const uint32_t* const r3 = rec0 + (i + 1) * kRowWords;
                const float ppN = __uint_as_float(r3[0]), ppJ = __uint_as_float(r3[1]), ppC = __uint_as_float(r3[2]);
                // lane 0's first state is node 1, which nothing but B enters: its gates are closed
                const float sM = shift1(M[S - 1]), sI = shift1(I[S - 1]), sD = shift1(D[S - 1]);
                uint32_t bits[S];
                float E = NINF;
#pragma unroll
                for (int q = S - 1; q >= 0; --q) {
                    const uint32_t g = gate(q);
                    const float ppm = mrow[q * kLanes], ppi = mrow[(S + q) * kLanes];
                    const float mi = (g & kGateMI) ? M[q] : NINF, ii = (g & kGateII) ? I[q] : NINF;
                    const float iv = fmaxf(mi, ii);
                    uint32_t b = iv == mi ? 0u : kIFromI;
                    const float pm = q ? M[q - 1] : sM, pi = q ? I[q - 1] : sI, pd = q ? D[q - 1] : sD;
                    const float cm = (g & kGateMM) ? pm : NINF, ci = (g & kGateIM) ? pi : NINF;
                    const float cd = (g & kGateDM) ? pd : NINF, cb = (g & kGateBM) ? B : NINF;
                    const float mx = fmaxf(fmaxf(cm, ci), fmaxf(cd, cb));
                    b |= mx == cm ? kFromM : mx == ci ? kFromI : mx == cd ? kFromD : kFromB;
                    M[q] = mx + ppm;
                    I[q] = iv + ppi;
                    E = fmaxf(E, M[q]);
                    bits[q] = b;
                }
                const float sMn = shift1(M[S - 1]);
                const float Eall = wave_max(E);
                uint32_t kmine = 0xffffffffu;
#pragma unroll
                for (int q = S - 1; q >= 0; --q)
                    if (M[q] == Eall) kmine = static_cast<uint32_t>(lane * S + q + 1);
                const uint32_t kE = wave_min(kmine);

                // D: each lane's chain from -inf, the lanes' outgoing values scanned, one max per open slot
#pragma unroll
                for (int q = 0; q < S; ++q) {
                    const uint32_t g = gate(q);
                    const float md = (g & kGateMD) ? (q ? M[q - 1] : sMn) : NINF;
                    const float dd = (q && (g & kGateDD)) ? D[q - 1] : NINF;
                    D[q] = fmaxf(md, dd);
                }
                float v = D[S - 1];
#pragma unroll
                for (int j = 0; j < kScanSteps; ++j) {
                    const float left = __shfl_up(v, 1 << j, 64);
                    v = fmaxf(v, ((steps >> j) & 1u) ? left : NINF);
                }
                const float up = __shfl_up(v, 1, 64);
                float Din = lane ? up : NINF;
#pragma unroll
                for (int q = 0; q < S; ++q) {
                    const uint32_t g = gate(q);
                    Din = (g & kGateDD) ? Din : NINF;  // the chain from the lane's edge, while it is open
                    D[q] = fmaxf(D[q], Din);
                    const float md = (g & kGateMD) ? (q ? M[q - 1] : sMn) : NINF;
                    if (!(D[q] == md)) bits[q] |= kDFromD;
                }
#pragma unroll
                for (int w = 0; w < W; ++w) {
                    uint32_t word = 0;
#pragma unroll
                    for (int c = 0; c < kCellsPerWord; ++c)
                        if (w * kCellsPerWord + c < S) word |= bits[w * kCellsPerWord + c] << (c * kCellBits);
                    ptrs[(i * W + w) * kLanes + lane] = word;
                }
                // specials, by every lane alike; the loop wins a tie with E, N with J
                const float Jl = J + ppJ, Cl = C + ppC;
                J = fmaxf(Jl, a.open_EJ ? Eall : NINF);
                C = fmaxf(Cl, a.open_EC ? Eall : NINF);
                N = N + ppN;
                const float Bn = open_move ? N : NINF;
                B = fmaxf(Bn, open_move ? J : NINF);
                if (lane == 0)
                    recs[i] = (kE & kRecKMask) | (C == Cl ? 0u : kRecCFromE) | (J == Jl ? 0u : kRecJFromE) |
                              (B == Bn ? 0u : kRecBFromJ);
            }
            if (lane == 0) a.oa_scores[s] = C;
        }
        item = seqq::next_item(a.counter, lane, nwaves);
    }
    seqq::last_exit<kFillWaves>(a.counter, &exited_s, lane);
}

// ------------------------------------------------------------------------------------------------
// The walk, one item per thread.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kWalkBlock) void aln_walk_kernel(const WalkArgs a) {
    using namespace vittrace;
    using namespace msv_host;
    const uint64_t j = static_cast<uint64_t>(blockIdx.x) * kWalkBlock + threadIdx.x;
    if (j >= a.hi - a.lo) return;
    const uint32_t s = a.lo + static_cast<uint32_t>(j);
    const uint64_t L = a.offsets[s + 1] - a.offsets[s];
    const bool write = a.domains != nullptr;
    uint32_t nd = 0;
    uint64_t no = 0;
    if (L != 0 && !not_finite(__float_as_uint(a.scores[s])) && !not_finite(__float_as_uint(a.oa_scores[s]))) {
        const uint32_t S = a.S, W = (S + kCellsPerWord - 1) / kCellsPerWord;
        const uint32_t* const rec0 = a.ws + a.base[s];
        const float* const mat = reinterpret_cast<const float*>(rec0 + aln_record_words(L));
        const uint32_t* const ptrs = rec0 + aln_record_words(L) + aln_matrix_words(S, L);
        const uint32_t* const recs = ptrs + L * (static_cast<uint64_t>(W) * kLanes);
        const msv_aln_item it = a.items[s];
        uint64_t dom_at = write ? a.dom_off[j + 1] : 0, ops_at = write ? a.ops_off[j + 1] : 0;
        aln_walk(
            L, S * kLanes,
            [&](uint64_t i, uint32_t k) -> uint32_t {
                const uint32_t v = (k - 1) / S, q = (k - 1) % S;
                return (ptrs[((i - 1) * W + q / kCellsPerWord) * kLanes + v] >> ((q % kCellsPerWord) * kCellBits)) & 15u;
            },
            [&](uint64_t i) -> uint32_t { return recs[i - 1]; },
            [&](char c, uint64_t i, uint32_t k) {
                ++no;
                if (write) {
                    const uint32_t v = (k - 1) / S, q = (k - 1) % S;
                    --ops_at;
                    a.ops[ops_at] = static_cast<uint8_t>(c);
                    a.op_pp[ops_at] = c == 'M'   ? mat[((i - 1) * 2 * S + q) * kLanes + v]
                                      : c == 'I' ? mat[((i - 1) * 2 * S + S + q) * kLanes + v]
                                                 : 0.0f;
                }
            },
            [&](uint32_t i_from, uint32_t i_to, uint32_t k_from, uint32_t k_to, uint32_t len) {
                ++nd;
                if (write) {
                    msv_vit_domain d;
                    d.seq = it.seq;
                    d.i_from = i_from + it.i_from - 1;
                    d.i_to = i_to + it.i_from - 1;
                    d.k_from = k_from;
                    d.k_to = k_to;
                    d.ops_len = len;
                    d.ops_begin = ops_at;
                    a.domains[--dom_at] = d;
                }
            });
    }
    if (!write) {
        a.counts[2 * j] = nd;
        a.counts[2 * j + 1] = static_cast<uint32_t>(no);
    }
}

// ------------------------------------------------------------------------------------------------
// Variant table: the domain stage's family, one recording / Backward pair per variant, one fill kernel per S.
// ------------------------------------------------------------------------------------------------
#define ALN_VARIANT(S_, ELDS_, ISC_, W_, NAME_)                                                         \
    AlnVariant{S_, ELDS_, ISC_, W_, reinterpret_cast<const void*>(&aln_fwd_kernel<S_, ELDS_, ISC_, W_>), \
               reinterpret_cast<const void*>(&aln_bck_kernel<S_, ELDS_, ISC_, W_>),                      \
               reinterpret_cast<const void*>(&aln_fill_kernel<S_>), NAME_}

const AlnVariant* aln_variants(int* count) {
    static const AlnVariant all[] = {
        ALN_VARIANT(2, true, false, 8, "aln_s2"),    ALN_VARIANT(6, true, false, 8, "aln_s6"),
        ALN_VARIANT(12, true, false, 8, "aln_s12"),  ALN_VARIANT(22, false, false, 8, "aln_s22g"),
        ALN_VARIANT(38, false, false, 4, "aln_s38g4"),
        ALN_VARIANT(2, true, true, 8, "aln_s2i"),    ALN_VARIANT(6, true, true, 8, "aln_s6i"),
        ALN_VARIANT(12, true, true, 8, "aln_s12i"),  ALN_VARIANT(22, false, true, 8, "aln_s22gi"),
        ALN_VARIANT(38, false, true, 4, "aln_s38g4i"),
    };
    *count = static_cast<int>(sizeof(all) / sizeof(all[0]));
    return all;
}

const void* walk_fn() { return reinterpret_cast<const void*>(&aln_walk_kernel); }

hipError_t aln_launch(const void* fn, int waves, uint32_t blocks, const AlnArgs& args, hipStream_t stream) {
    void* params[] = {const_cast<AlnArgs*>(&args)};
    return hipLaunchKernel(fn, dim3(blocks), dim3(waves * 64), params, 0, stream);
}

hipError_t launch_walk(const WalkArgs& a, hipStream_t stream) {
    if (a.hi <= a.lo) return hipSuccess;
    hipLaunchKernelGGL(aln_walk_kernel, dim3((a.hi - a.lo + kWalkBlock - 1) / kWalkBlock), dim3(kWalkBlock), 0, stream,
                       a);
    return hipGetLastError();
}

}  // namespace alnk
