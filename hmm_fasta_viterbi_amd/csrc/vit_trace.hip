// vit_trace.hip -- the Viterbi trace on gfx950 (msv.h "Viterbi traces"): a fill kernel that runs
// vit_kernel.hip's recurrence and writes 4 source bits per cell while the row is in registers, and a walk
// kernel that follows them back from C(L).  This is the path of the hits, not of the database: it is built for
// exactness and plainness, not for throughput.
//
// Fill (one kernel per plan of vit_trace_plan.h):
//   * one sequence per WORKGROUP of `team` waves; lane v = wave * 64 + lane holds the S consecutive states
//     v * S + 1 .. v * S + S of M, I, D in VGPRs, the 7 transition arrays beside them (vit_tables' team layout,
//     match and insert scores read from L2 every row);
//   * residues as vit_kernel.hip: one byte per lane per 64-row block, a block ahead, v_readlane per row (each
//     wave keeps its own copy of the block);
//   * every value that crosses a lane boundary -- the previous row's last M / I / D, this row's last M, and the D
//     chain -- goes through LDS with a workgroup barrier, the same code inside a wave and across waves.  The D
//     chain is lazy-F over the whole workgroup: each lane starts its chain from -inf, then while any lane's
//     incoming D(k-1) + tDD beats its first D (__syncthreads_or) the lanes re-run their chains.  Lower bounds only
//     rise to the exact value, so the result is the serial chain bit for bit;
//   * a cell's sources are found by equality on FINAL values, candidates in msv.h's tie-break order -- for D
//     after lazy-F has converged -- so the bits are the serial DP's (msv_host::viterbi_trace_on_sequence);
//   * E's argmax is a workgroup max, then the smallest k holding it (a workgroup min over the lanes' first
//     matching slot); J, C, N, B are then computed by every lane alike, and lane 0 writes the row's record;
//   * the grid is persistent, its queue seq_queue.h's with a workgroup as the worker (no select_count, no idle exit).
// Rows never live in scratch: the row arrays are indexed by unrolled constants only.
#include <hip/hip_runtime.h>

#include "msv_kernel_impl.h"
#include "seq_queue.h"
#include "vit_kernel.h"
#include "vit_trace.h"
#include "vit_trace_plan.h"

namespace vittrace {

namespace {

using vitk::DD_IN;
using vitk::DM_IN;
using vitk::II;
using vitk::IM_IN;
using vitk::kRows;
using vitk::kTransitions;
using vitk::MD_IN;
using vitk::MI;
using vitk::MM_IN;

constexpr float NINF = -__builtin_inff();

using seqq::u64first;

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

}  // namespace

template <int S, int T>
__global__ __launch_bounds__(T * 64) void vit_trace_fill(const FillArgs a) {
    static_assert(S % 8 == 0, "whole pointer words per lane");
    constexpr int C2 = S / 2, VL = T * 64, W = S / kCellsPerWord;
    __shared__ float xM[VL], xI[VL], xD[VL], xMn[VL], xDn[VL];  // a lane's last state, for the lane on its right
    __shared__ float redE[T];
    __shared__ uint32_t redK[T];
    __shared__ uint32_t next_s;
    const int vl = threadIdx.x, lane = vl & 63;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);

    float tr[kTransitions][S];
#pragma unroll
    for (int j = 0; j < kTransitions; ++j)
#pragma unroll
        for (int c = 0; c < C2; ++c) {
            const float2 t = a.ttab[(j * C2 + c) * VL + vl];
            tr[j][2 * c] = t.x;
            tr[j][2 * c + 1] = t.y;
        }
    const bool isc = a.itab != nullptr;  // (uniform)

    uint32_t item = blockIdx.x;
    while (item < a.n_items) {
        const uint32_t s = __builtin_amdgcn_readfirstlane(a.select[item]);
        const uint64_t o0 = u64first(a.offsets[s]);
        const uint64_t L = u64first(a.offsets[s + 1]) - o0;
        if (L == 0) {
            if (vl == 0) a.scores[item] = NINF;  // C_0 = -inf
        } else if (L >= a.lentab_n) {
            if (vl == 0) {
                a.scores[item] = __uint_as_float(0x7fc00000u);
                atomicOr(a.errors, msvk::kErrTooLong);
            }
        } else {
            const float2 lm = a.lentab[L];
            const float loop = lm.x, move = lm.y;
            uint32_t* const ptrs = a.ws + a.base[item];
            uint32_t* const recs = ptrs + L * (static_cast<uint64_t>(W) * VL);
            float M[S], I[S], D[S];
#pragma unroll
            for (int q = 0; q < S; ++q) M[q] = I[q] = D[q] = NINF;
            float J = NINF, C = NINF, N = 0.0f, B = move;
            uint32_t maxcode = 0;
            const uint8_t* res = a.residues + o0;
            uint32_t cur = static_cast<uint64_t>(lane) < L ? res[lane] : 0u;
            uint32_t nxt = static_cast<uint64_t>(64 + lane) < L ? res[64 + lane] : 0u;
            for (uint64_t i = 0; i < L; ++i) {
                const uint32_t ph = static_cast<uint32_t>(i) & 63u;
                if (ph == 0 && i != 0) {
                    cur = nxt;
                    nxt = (i + 64 + lane < L) ? res[i + 64 + lane] : 0u;
                }
                uint32_t code = __builtin_amdgcn_readlane(cur, ph);
                maxcode = code > maxcode ? code : maxcode;
                code = code < 19u ? code : 19u;
                const float2* er = a.etab + code * (C2 * VL) + vl;
                const float2* ir = isc ? a.itab + code * (C2 * VL) + vl : nullptr;

                // the previous row's last states, from the lane on the left (k - 1 across the boundary)
                xM[vl] = M[S - 1];
                xI[vl] = I[S - 1];
                xD[vl] = D[S - 1];
                __syncthreads();
                const float sM = vl ? xM[vl - 1] : NINF, sI = vl ? xI[vl - 1] : NINF, sD = vl ? xD[vl - 1] : NINF;

                const float Bt = B + a.tr_B_Mk;
                uint32_t bits[S];
                float E = NINF;
                // M/I pass, highest slot first: every register is updated in place
#pragma unroll
                for (int c = C2 - 1; c >= 0; --c) {
                    const float2 e2 = er[c * VL];
                    float2 i2 = make_float2(0.0f, 0.0f);
                    if (isc) i2 = ir[c * VL];
#pragma unroll
                    for (int h = 1; h >= 0; --h) {
                        const int q = 2 * c + h;
                        const float mi = M[q] + tr[MI][q], ii = I[q] + tr[II][q];
                        float iv = fmaxf(mi, ii);
                        uint32_t b = iv == mi ? 0u : kIFromI;
                        if (isc) iv = iv + (h ? i2.y : i2.x);
                        const float pm = q ? M[q - 1] : sM, pi = q ? I[q - 1] : sI, pd = q ? D[q - 1] : sD;
                        const float cm = pm + tr[MM_IN][q], ci = pi + tr[IM_IN][q], cd = pd + tr[DM_IN][q];
                        const float mx = fmaxf(fmaxf(cm, ci), fmaxf(cd, Bt));
                        b |= mx == cm ? kFromM : mx == ci ? kFromI : mx == cd ? kFromD : kFromB;
                        M[q] = mx + (h ? e2.y : e2.x);
                        I[q] = iv;
                        E = fmaxf(E, M[q]);
                        bits[q] = b;
                    }
                }
                // this row's M(k-1) for each lane's first D, and the workgroup's E
                xMn[vl] = M[S - 1];
                const float Ew = wave_max(E);
                if (lane == 0) redE[wave] = Ew;
                __syncthreads();
                const float sMn = vl ? xMn[vl - 1] : NINF;
                float Eall = redE[0];
#pragma unroll
                for (int w = 1; w < T; ++w) Eall = fmaxf(Eall, redE[w]);
                // the smallest k with M(i,k) == E(i)
                uint32_t kmine = 0xffffffffu;
#pragma unroll
                for (int q = S - 1; q >= 0; --q)
                    if (M[q] == Eall) kmine = static_cast<uint32_t>(vl * S + q + 1);
                const uint32_t kw = wave_min(kmine);
                if (lane == 0) redK[wave] = kw;

                // D pass, lowest slot first, each lane's chain started from -inf ...
                D[0] = sMn + tr[MD_IN][0];
#pragma unroll
                for (int q = 1; q < S; ++q) D[q] = fmaxf(M[q - 1] + tr[MD_IN][q], D[q - 1] + tr[DD_IN][q]);
                // ... and lazy-F over the workgroup's lanes until no lane's first state changes
                float sDn;
                for (;;) {
                    xDn[vl] = D[S - 1];
                    __syncthreads();
                    sDn = vl ? xDn[vl - 1] : NINF;
                    const float cand = sDn + tr[DD_IN][0];
                    if (!__syncthreads_or(cand > D[0])) break;
                    D[0] = fmaxf(D[0], cand);
#pragma unroll
                    for (int q = 1; q < S; ++q) D[q] = fmaxf(D[q], D[q - 1] + tr[DD_IN][q]);
                }
                // D's source on the final values (sDn is the left lane's final last D): M before D
                if (!(D[0] == sMn + tr[MD_IN][0])) bits[0] |= kDFromD;
#pragma unroll
                for (int q = 1; q < S; ++q)
                    if (!(D[q] == M[q - 1] + tr[MD_IN][q])) bits[q] |= kDFromD;

                // the row's back-pointers: [row][word][lane], a wave's store is one contiguous line
#pragma unroll
                for (int w = 0; w < W; ++w) {
                    uint32_t word = 0;
#pragma unroll
                    for (int c = 0; c < kCellsPerWord; ++c) word |= bits[w * kCellsPerWord + c] << (c * kCellBits);
                    ptrs[(i * W + w) * VL + vl] = word;
                }

                // specials (MSV_HMM.cpp:107-110), by every lane alike; the loop wins a tie with E, N with J.
                // (redK was written before the lazy-F barriers, so it is complete here; the next row's writes of
                // redE / redK come after that row's first barrier, which every lane reaches after these reads)
                uint32_t kE = redK[0];
#pragma unroll
                for (int w = 1; w < T; ++w) kE = redK[w] < kE ? redK[w] : kE;
                const float Jl = J + loop, Cl = C + loop;
                J = fmaxf(Jl, Eall + a.tr_E_J);
                C = fmaxf(Cl, Eall + a.tr_E_C);
                N = N + loop;
                const float Bn = N + move;
                B = fmaxf(Bn, J + move);
                if (vl == 0)
                    recs[i] = (kE & kRecKMask) | (C == Cl ? 0u : kRecCFromE) | (J == Jl ? 0u : kRecJFromE) |
                              (B == Bn ? 0u : kRecBFromJ);
            }
            // every wave saw every residue, so maxcode is the same in all of them
            if (vl == 0) {
                if (maxcode >= 20u) {
                    a.scores[item] = __builtin_inff();
                    atomicOr(a.errors, msvk::kErrBadResidue);
                } else {
                    a.scores[item] = C + move;
                }
            }
        }
        __syncthreads();  // (the previous read of next_s, and this item's LDS reads, are over)
        if (vl == 0) next_s = gridDim.x + atomicAdd(a.counter, 1u);
        __syncthreads();
        item = next_s;
    }
    // the last workgroup to finish resets the counters for the next launch on this slot
    if (vl == 0) {
        __threadfence();
        seqq::count_leavers<1, 1>(a.counter);
    }
}

// One lane per item.  Every step lowers i or k, so the walk ends after at most L + LENG steps whatever the
// workspace holds; the pointers of a finite score lead through finite cells only, so i and k stay >= 1 on them.
__global__ __launch_bounds__(64) void vit_trace_walk(const WalkArgs a) {
    const uint32_t j = blockIdx.x * 64 + threadIdx.x;
    if (j >= a.n_items) return;
    const uint32_t s = a.select[j];
    const uint64_t L = a.offsets[s + 1] - a.offsets[s];
    const float score = a.scores[j];
    const bool write = a.domains != nullptr;
    uint32_t nd = 0;
    uint64_t no = 0;
    uint64_t dom_at = write ? a.dom_off[j + 1] : 0, ops_at = write ? a.ops_off[j + 1] : 0;  // written backwards
    // a finite score (by its exponent bits): an empty, bad or too long sequence has no domains
    if (L != 0 && (__float_as_uint(score) & 0x7f800000u) != 0x7f800000u) {
        const uint64_t row = static_cast<uint64_t>(a.words) * a.lanes;
        const uint32_t* const ptrs = a.ws + a.base[j];
        const uint32_t* const recs = ptrs + L * row;
        uint64_t i = L;
        while (i >= 1 && !(recs[i - 1] & kRecCFromE)) --i;  // C loops
        while (i >= 1) {
            uint32_t k = recs[i - 1] & kRecKMask;  // E(i) -> M(i, k)
            const uint32_t i_to = static_cast<uint32_t>(i), k_to = k;
            uint32_t i_from = 0, k_from = 0, len = 0;
            int st = 0;  // 0 M, 1 I, 2 D
            bool entered = false;
            while (!entered && i >= 1 && k >= 1 && k <= a.S * a.lanes) {
                const uint32_t v = (k - 1) / a.S, q = (k - 1) % a.S;
                const uint32_t word = ptrs[((i - 1) * a.words + q / kCellsPerWord) * a.lanes + v];
                const uint32_t b = (word >> ((q % kCellsPerWord) * kCellBits)) & 15u;
                uint8_t op;
                if (st == 0) {
                    op = 'M';
                    const uint32_t src = b & 3u;
                    if (src == kFromB) {
                        entered = true;
                        i_from = static_cast<uint32_t>(i);
                        k_from = k;
                    } else {
                        st = src == kFromM ? 0 : src == kFromI ? 1 : 2;
                    }
                    --i;
                    --k;
                } else if (st == 1) {
                    op = 'I';
                    st = (b & kIFromI) ? 1 : 0;
                    --i;
                } else {
                    op = 'D';
                    st = (b & kDFromD) ? 2 : 0;
                    --k;
                }
                ++len;
                if (write) a.ops[--ops_at] = op;
            }
            ++nd;
            no += len;
            if (write) {
                msv_vit_domain d;
                d.seq = s;
                d.i_from = i_from;
                d.i_to = i_to;
                d.k_from = k_from;
                d.k_to = k_to;
                d.ops_len = len;
                d.ops_begin = ops_at;
                a.domains[--dom_at] = d;
            }
            // B(i): from N (the path's start) or from J, which loops back to an earlier E
            if (!entered || i == 0 || !(recs[i - 1] & kRecBFromJ)) break;
            while (i >= 1 && !(recs[i - 1] & kRecJFromE)) --i;
        }
    }
    if (!write) {
        a.counts[2 * j] = nd;
        // (n_ops <= L + LENG per domain chain: a sequence's ops fit 32 bits while L < 2^31 and LENG <= 4096)
        a.counts[2 * j + 1] = static_cast<uint32_t>(no);
    }
}

namespace {
template <int I>
const void* fill_fn() {
    return reinterpret_cast<const void*>(&vit_trace_fill<kPlans[I].S, kPlans[I].team>);
}
}  // namespace

const void* fill_kernel(int plan) {
    static_assert(kPlanCount == 3, "one instantiation per plan");
    switch (plan) {
        case 0: return fill_fn<0>();
        case 1: return fill_fn<1>();
        case 2: return fill_fn<2>();
    }
    return nullptr;
}

hipError_t launch_fill(int plan, uint32_t blocks, const FillArgs& a, hipStream_t stream) {
    const void* fn = fill_kernel(plan);
    if (!fn) return hipErrorInvalidValue;
    void* params[] = {const_cast<FillArgs*>(&a)};
    return hipLaunchKernel(fn, dim3(blocks), dim3(kPlans[plan].lanes()), params, 0, stream);
}

hipError_t launch_walk(const WalkArgs& a, hipStream_t stream) {
    if (a.n_items == 0) return hipSuccess;
    hipLaunchKernelGGL(vit_trace_walk, dim3((a.n_items + 63) / 64), dim3(64), 0, stream, a);
    return hipGetLastError();
}

}  // namespace vittrace
