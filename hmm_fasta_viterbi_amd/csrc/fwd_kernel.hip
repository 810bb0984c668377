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
#include <hip/hip_runtime.h>

#include "fwd_host.h"
#include "fwd_kernel.h"
#include "msv_kernel.h"
#include "seq_queue.h"

namespace fwdk {

namespace {

// Lane l-1's value into lane l, 0 into lane 0: one DPP move across the wave (wave_shr:1, bound_ctrl off: the
// lane without a source keeps `old`, which is 0).
constexpr int DPP_WAVE_SHR1 = 0x138;
__device__ __forceinline__ float shift1(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), DPP_WAVE_SHR1, 0xF, 0xF, false));
}
// Lane l-d's value into lane l (d = 2 .. 32), 0 into lanes below d: ds_bpermute_b32 (the LDS crossbar, no LDS
// memory) and a select.
__device__ __forceinline__ float shift_by(float v, int lane, int d) {
    const float t = __int_as_float(__builtin_amdgcn_ds_bpermute((lane - d) * 4, __float_as_int(v)));
    return lane >= d ? t : 0.0f;
}
// The 64-lane sum as a butterfly: every lane adds the same pairs in the same order, so all lanes hold the same
// bits (a + b == b + a).
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

}  // namespace

template <int S, bool ELDS, bool ISC, int WAVES>
__global__ __launch_bounds__(WAVES * 64) void fwd_kernel(const FwdArgs a) {
    static_assert(S >= 2 && S % 2 == 0, "S must be even");
    constexpr int C2 = S / 2;
    constexpr int ROW2 = C2 * kLanes;  // float2 per table row
    // long rows: every chunk its own scheduling region, or the scheduler hoists a whole row of loads and spills
    constexpr bool FENCE = S > 12;
    __shared__ float2 etab_s[ELDS ? kRows * ROW2 : 1];
    __shared__ float2 ttab_s[kArrays * ROW2];
    __shared__ uint32_t exited_s;
    const int lane = threadIdx.x & 63;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t total = seqq::list_total(a);
    if (static_cast<uint64_t>(blockIdx.x) * WAVES >= total) {
        // no sequence for this workgroup (a device-count launch is sized for n): leave, counted like any other
        if (threadIdx.x == 0) seqq::count_leavers<1, 1>(a.counter);
        return;
    }

    if constexpr (ELDS)
        for (int i = threadIdx.x; i < kRows * ROW2; i += WAVES * 64) etab_s[i] = a.etab[i];
    for (int i = threadIdx.x; i < kArrays * ROW2; i += WAVES * 64) ttab_s[i] = a.ttab[i];
    if (threadIdx.x == 0) exited_s = 0;
    __syncthreads();

    float A[kScanSteps];  // this lane's multiplier of every scan step, in VGPRs for the whole launch
#pragma unroll
    for (int j = 0; j < kScanSteps; ++j) A[j] = a.scan[j * kLanes + lane];
    // `rz` is an opaque zero renewed every row: without it the compiler hoists the loop-invariant LDS loads of
    // the slot arrays out of the row loop into VGPRs and spills them
    uint32_t rz = 0;
    auto tlds = [&](int j, int c) -> float2 { return ttab_s[rz + (j * C2 + c) * kLanes + lane]; };

    const uint32_t nwaves = gridDim.x * WAVES;
    uint32_t item = blockIdx.x * WAVES + wave;
    while (item < total) {
        uint32_t s;
        uint64_t o0, L;
        if (seqq::take(a, item, lane, &s, &o0, &L)) {
            const float2 lm = a.lentab[L];
            const float loop = lm.x, move = lm.y;
            // everything a sequence carries starts here: M, I, D, the specials and the scale's exponent
            float M[S], I[S], D[S];
#pragma unroll
            for (int q = 0; q < S; ++q) M[q] = I[q] = D[q] = 0.0f;
            float N = 1.0f, J = 0.0f, Cc = 0.0f, B = move;
            int32_t e2 = 0;  // the values are the true ones times 2^-e2
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
                asm volatile("" : "+v"(rz));
                const float Bt = B * a.tBM;
                const float2* er;
                if constexpr (ELDS) er = etab_s + code * ROW2 + lane;
                else er = a.etab + code * ROW2 + lane;
                const float2* ir = a.itab + code * ROW2 + lane;

                // the previous row's last states, from the lane on the left (k - 1 across the boundary)
                const float sM = shift1(M[S - 1]), sI = shift1(I[S - 1]), sD = shift1(D[S - 1]);
                // M/I pass, highest slot first, in place: I(k) reads M'(k), I'(k); M(k) reads M'(k-1), I'(k-1),
                // D'(k-1).  The B term is added last.
                float Es = 0.0f;
#pragma unroll
                for (int c = C2 - 1; c >= 0; --c) {
                    const float2 tmm = tlds(MM_IN, c), tim = tlds(IM_IN, c), tdm = tlds(DM_IN, c);
                    const float2 tmi = tlds(MI, c), tii = tlds(II, c);
                    const float2 e = er[c * kLanes];
                    float2 ins = {1.0f, 1.0f};
                    if constexpr (ISC) ins = ir[c * kLanes];
#pragma unroll
                    for (int h = 1; h >= 0; --h) {
                        const int q = 2 * c + h;
                        float iv = fmaf(I[q], h ? tii.y : tii.x, M[q] * (h ? tmi.y : tmi.x));
                        if constexpr (ISC) iv = iv * (h ? ins.y : ins.x);
                        const float pm = q ? M[q - 1] : sM, pi = q ? I[q - 1] : sI, pd = q ? D[q - 1] : sD;
                        const float acc = fmaf(pd, h ? tdm.y : tdm.x,
                                               fmaf(pi, h ? tim.y : tim.x, pm * (h ? tmm.y : tmm.x)));
                        const float m = (h ? e.y : e.x) * (acc + Bt);
                        M[q] = m;
                        I[q] = iv;
                        Es += m;
                    }
                    if constexpr (FENCE) __builtin_amdgcn_sched_barrier(0);
                }
                // D pass, lowest slot first, each lane's chain started from an incoming 0
                const float sMn = shift1(M[S - 1]);  // this row's M(k-1) for each lane's first slot
#pragma unroll
                for (int c = 0; c < C2; ++c) {
                    const float2 tmd = tlds(MD_IN, c), tdd = tlds(DD_IN, c);
                    D[2 * c] = c ? fmaf(D[2 * c - 1], tdd.x, M[2 * c - 1] * tmd.x) : sMn * tmd.x;
                    D[2 * c + 1] = fmaf(D[2 * c], tdd.y, M[2 * c] * tmd.y);
                    if constexpr (FENCE) __builtin_amdgcn_sched_barrier(0);
                }
                // the lanes' affine maps D_out = a D_in + b, scanned inclusively over the lanes: after step j,
                // b is the lane's last D given an incoming 0 at lane l - 2^(j+1) + 1
                float b = D[S - 1];
                b = fmaf(A[0], shift1(b), b);
#pragma unroll
                for (int j = 1; j < kScanSteps; ++j) b = fmaf(A[j], shift_by(b, lane, 1 << j), b);
                const float Din = shift1(b);  // the exact D entering this lane (0 into lane 0)
#pragma unroll
                for (int c = 0; c < C2; ++c) {
                    const float2 dc = tlds(DC, c);
                    D[2 * c] = fmaf(Din, dc.x, D[2 * c]);
                    D[2 * c + 1] = fmaf(Din, dc.y, D[2 * c + 1]);
                    Es += D[2 * c];
                    Es += D[2 * c + 1];
                    if constexpr (FENCE) __builtin_amdgcn_sched_barrier(0);
                }
                // specials: E is the same in every lane (wave_sum), so J, C, N, B and the rescaling are uniform
                const float E = wave_sum(Es);
                N = N * loop;
                J = fmaf(J, loop, E * a.tEJ);
                Cc = fmaf(Cc, loop, E * a.tEC);
                B = (N + J) * move;
                const uint32_t Eb = __builtin_amdgcn_readfirstlane(__float_as_uint(E));  // (E >= 0: bits order as floats)
                if (Eb > 0x4f800000u && Eb < 0x7f800000u) {  // 2^32 < E < inf
                    // scale down by 2^-x, x = E's exponent (at most 126, so 2^-x is a normal float): exact
                    uint32_t x = (Eb >> 23) - 127u;
                    x = x < 126u ? x : 126u;
                    const float down = __uint_as_float((127u - x) << 23);
#pragma unroll
                    for (int q = 0; q < S; ++q) {
                        M[q] *= down;
                        I[q] *= down;
                        D[q] *= down;
                    }
                    N *= down;
                    J *= down;
                    Cc *= down;
                    B *= down;
                    e2 += static_cast<int32_t>(x);
                }
            }
            const float sc = fmaf(static_cast<float>(e2), 0.69314718055994529f, logf(Cc * move));
            if (lane == 0) {
                if (maxcode >= 20u) {
                    a.scores[s] = __builtin_inff();
                    atomicOr(a.errors, msvk::kErrBadResidue);
                } else {
                    a.scores[s] = sc;
                }
            }
        }
        uint32_t t = 0;
        if (lane == 0) t = atomicAdd(a.counter, 1u);
        item = nwaves + __builtin_amdgcn_readfirstlane(t);
    }
    // the last workgroup to finish resets the counters for the next launch on this profile (one grid-level
    // atomic per workgroup, by its last wave, counted in LDS)
    if (lane == 0) {
        __threadfence();
        if (atomicAdd(&exited_s, 1u) == WAVES - 1) seqq::count_leavers<1, 1>(a.counter);
    }
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
