// dom_kernel.hip -- the domain stage on gfx950: Backward, the per-residue domain posteriors that
// come from Forward x Backward on the special states, and the envelope rule.  msv.h states the model.
//
// Two persistent launches per chunk of selected sequences, both in fwd_kernel.hip's shape (one sequence per 64-lane
// wave, lane l holds the S consecutive states l*S+1 .. l*S+S, wave-uniform residues in 64-row blocks, the work
// queue of seq_queue.h) and with its table placement per S:
//   dom_fwd_kernel  Forward's row restated (fwd_kernel.hip itself is untouched); after every row lane 0 stores the
//                   row's N, J, C, B, E and the running exponent -- six words, row 0 included -- to the workspace.
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
#include "seq_queue.h"

namespace domk {

namespace {

// Lane l-1's value into lane l, 0 into lane 0 (wave_shr:1), and lane l+1's value into lane l, 0 into lane 63
// (wave_shl:1): one DPP move across the wave each, bound_ctrl off (the lane without a source keeps `old`, 0).
constexpr int DPP_WAVE_SHR1 = 0x138;
constexpr int DPP_WAVE_SHL1 = 0x130;
__device__ __forceinline__ float shift1(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), DPP_WAVE_SHR1, 0xF, 0xF, false));
}
__device__ __forceinline__ float shift1_down(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), DPP_WAVE_SHL1, 0xF, 0xF, false));
}
// Lane l-d's value into lane l, 0 into lanes below d; lane l+d's value into lane l, 0 into lanes above 63-d.
__device__ __forceinline__ float shift_by(float v, int lane, int d) {
    const float t = __int_as_float(__builtin_amdgcn_ds_bpermute((lane - d) * 4, __float_as_int(v)));
    return lane >= d ? t : 0.0f;
}
__device__ __forceinline__ float shift_down_by(float v, int lane, int d) {
    const float t = __int_as_float(__builtin_amdgcn_ds_bpermute(((lane + d) & 63) * 4, __float_as_int(v)));
    return lane + d < kLanes ? t : 0.0f;
}
// The 64-lane sum as a butterfly: all lanes hold the same bits.
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// The first workspace row of list entry `item` (sequence s, first residue o0)
__device__ __forceinline__ uint64_t first_row(const DomArgs& a, uint32_t item, uint32_t s, uint64_t o0) {
    return a.item_rows ? seqq::u64first(a.item_rows[item]) : o0 + s;
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// The recording Forward kernel: fwd_kernel.hip's body, statement for statement, plus the record stores.
// ------------------------------------------------------------------------------------------------
template <int S, bool ELDS, bool ISC, int WAVES>
__global__ __launch_bounds__(WAVES * 64) void dom_fwd_kernel(const DomArgs a) {
    static_assert(S >= 2 && S % 2 == 0, "S must be even");
    constexpr int C2 = S / 2;
    constexpr int ROW2 = C2 * kLanes;
    constexpr bool FENCE = S > 12;
    enum : int { MM_IN = 0, IM_IN = 1, DM_IN = 2, MI = 3, II = 4, MD_IN = 5, DD_IN = 6, DC = 7 };  // fwdk::
    __shared__ float2 etab_s[ELDS ? kRows * ROW2 : 1];
    __shared__ float2 ttab_s[kArrays * ROW2];
    __shared__ uint32_t exited_s;
    const int lane = threadIdx.x & 63;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t total = seqq::list_total(a);
    if (static_cast<uint64_t>(blockIdx.x) * WAVES >= total) {
        if (threadIdx.x == 0) seqq::count_leavers<1, 1>(a.counter);
        return;
    }

    if constexpr (ELDS)
        for (int i = threadIdx.x; i < kRows * ROW2; i += WAVES * 64) etab_s[i] = a.etab[i];
    for (int i = threadIdx.x; i < kArrays * ROW2; i += WAVES * 64) ttab_s[i] = a.ttab[i];
    if (threadIdx.x == 0) exited_s = 0;
    __syncthreads();

    float A[kScanSteps];
#pragma unroll
    for (int j = 0; j < kScanSteps; ++j) A[j] = a.scan[j * kLanes + lane];
    uint32_t rz = 0;  // an opaque zero renewed every row (fwd_kernel.hip)
    auto tlds = [&](int j, int c) -> float2 { return ttab_s[rz + (j * C2 + c) * kLanes + lane]; };

    const uint32_t nwaves = gridDim.x * WAVES;
    uint32_t item = blockIdx.x * WAVES + wave;
    while (item < total) {
        uint32_t s;
        uint64_t o0, L;
        if (seqq::take(a, item, lane, &s, &o0, &L)) {
            const float2 lm = a.lentab[L];
            const float loop = lm.x, move = lm.y;
            float M[S], I[S], D[S];
#pragma unroll
            for (int q = 0; q < S; ++q) M[q] = I[q] = D[q] = 0.0f;
            float N = 1.0f, J = 0.0f, Cc = 0.0f, B = move;
            int32_t e2 = 0;
            uint32_t maxcode = 0;
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

                const float sM = shift1(M[S - 1]), sI = shift1(I[S - 1]), sD = shift1(D[S - 1]);
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
                const float sMn = shift1(M[S - 1]);
#pragma unroll
                for (int c = 0; c < C2; ++c) {
                    const float2 tmd = tlds(MD_IN, c), tdd = tlds(DD_IN, c);
                    D[2 * c] = c ? fmaf(D[2 * c - 1], tdd.x, M[2 * c - 1] * tmd.x) : sMn * tmd.x;
                    D[2 * c + 1] = fmaf(D[2 * c], tdd.y, M[2 * c] * tmd.y);
                    if constexpr (FENCE) __builtin_amdgcn_sched_barrier(0);
                }
                float b = D[S - 1];
                b = fmaf(A[0], shift1(b), b);
#pragma unroll
                for (int j = 1; j < kScanSteps; ++j) b = fmaf(A[j], shift_by(b, lane, 1 << j), b);
                const float Din = shift1(b);
#pragma unroll
                for (int c = 0; c < C2; ++c) {
                    const float2 dc = tlds(DC, c);
                    D[2 * c] = fmaf(Din, dc.x, D[2 * c]);
                    D[2 * c + 1] = fmaf(Din, dc.y, D[2 * c + 1]);
                    Es += D[2 * c];
                    Es += D[2 * c + 1];
                    if constexpr (FENCE) __builtin_amdgcn_sched_barrier(0);
                }
                float E = wave_sum(Es);
                N = N * loop;
                J = fmaf(J, loop, E * a.tEJ);
                Cc = fmaf(Cc, loop, E * a.tEC);
                B = (N + J) * move;
                const uint32_t Eb = __builtin_amdgcn_readfirstlane(__float_as_uint(E));
                if (Eb > 0x4f800000u && Eb < 0x7f800000u) {  // 2^32 < E < inf
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
                    E *= down;  // (recorded only)
                    e2 += static_cast<int32_t>(x);
                }
                record(E);  // row i + 1, in the scale of its exponent
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
    if (lane == 0) {
        __threadfence();
        if (atomicAdd(&exited_s, 1u) == WAVES - 1) seqq::count_leavers<1, 1>(a.counter);
    }
}

// ------------------------------------------------------------------------------------------------
// Backward with the posteriors.
// ------------------------------------------------------------------------------------------------
template <int S, bool ELDS, bool ISC, int WAVES>
__global__ __launch_bounds__(WAVES * 64) void dom_bck_kernel(const DomArgs a) {
    static_assert(S >= 2 && S % 2 == 0, "S must be even");
    constexpr int C2 = S / 2;
    constexpr int ROW2 = C2 * kLanes;
    constexpr bool FENCE = S > 12;
    __shared__ float2 etab_s[ELDS ? kRows * ROW2 : 1];
    __shared__ float2 ttab_s[kArrays * ROW2];
    __shared__ uint32_t exited_s;
    const int lane = threadIdx.x & 63;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t total = seqq::list_total(a);
    if (static_cast<uint64_t>(blockIdx.x) * WAVES >= total) {
        if (threadIdx.x == 0) seqq::count_leavers<1, 1>(a.counter);
        return;
    }

    if constexpr (ELDS)
        for (int i = threadIdx.x; i < kRows * ROW2; i += WAVES * 64) etab_s[i] = a.etab[i];
    for (int i = threadIdx.x; i < kArrays * ROW2; i += WAVES * 64) ttab_s[i] = a.ttab[i];
    if (threadIdx.x == 0) exited_s = 0;
    __syncthreads();

    float A[kScanSteps];  // this lane's multiplier of every scan step
#pragma unroll
    for (int j = 0; j < kScanSteps; ++j) A[j] = a.scan[j * kLanes + lane];
    uint32_t rz = 0;
    auto tlds = [&](int j, int c) -> float2 { return ttab_s[rz + (j * C2 + c) * kLanes + lane]; };

    const uint32_t nwaves = gridDim.x * WAVES;
    uint32_t item = blockIdx.x * WAVES + wave;
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
                // everything a sequence carries starts here: bM, bI of the row below, the specials, the exponent
                float M[S], I[S], D[S];
#pragma unroll
                for (int q = 0; q < S; ++q) M[q] = I[q] = D[q] = 0.0f;
                float bJ = 0.0f, bC = 0.0f, bN = 0.0f;
                int32_t e2 = 0;  // the values are the true ones times 2^-e2
                const uint8_t* res = a.residues + o0;
                // residues in 64-row blocks from the back: `cur` holds the block of row i's residue (index i)
                const uint64_t top = (L - 1) >> 6;
                uint32_t cur = (top * 64 + lane < L) ? res[top * 64 + lane] : 0u;
                uint32_t nxt = top ? res[(top - 1) * 64 + lane] : 0u;
                float bNout = 0.0f;
                for (uint64_t i = L + 1; i-- > 0;) {
                    // this row's Forward record, asked for before the row's first pass
                    const uint32_t* const r6 = rec0 + i * kRowWords;
                    const float fN = __uint_as_float(r6[0]), fJ = __uint_as_float(r6[1]), fC = __uint_as_float(r6[2]);
                    const float fB = __uint_as_float(r6[3]), fE = __uint_as_float(r6[4]);
                    const int32_t ef = static_cast<int32_t>(r6[5]);
                    uint32_t code = 0;
                    if (i < L) {
                        const uint32_t ph = static_cast<uint32_t>(i) & 63u;
                        if (ph == 63u && i != L - 1) {
                            cur = nxt;
                            nxt = (i >= 127) ? res[((i >> 6) - 1) * 64 + lane] : 0u;
                        }
                        code = __builtin_amdgcn_readlane(cur, ph);
                        code = code < 19u ? code : 19u;
                    }
                    asm volatile("" : "+v"(rz));
                    const float2* er;
                    if constexpr (ELDS) er = etab_s + code * ROW2 + lane;
                    else er = a.etab + code * ROW2 + lane;
                    const float2* ir = a.itab + code * ROW2 + lane;

                    // P(k) = m bM'(k) in M's registers, H(k) = ins bI'(k) in I's; the lanes' sums of P
                    float Ps = 0.0f;
#pragma unroll
                    for (int c = 0; c < C2; ++c) {
                        const float2 e = er[c * kLanes];
                        M[2 * c] = e.x * M[2 * c];
                        M[2 * c + 1] = e.y * M[2 * c + 1];
                        Ps += M[2 * c];
                        Ps += M[2 * c + 1];
                        if constexpr (ISC) {
                            const float2 ins = ir[c * kLanes];
                            I[2 * c] = ins.x * I[2 * c];
                            I[2 * c + 1] = ins.y * I[2 * c + 1];
                        }
                        if constexpr (FENCE) __builtin_amdgcn_sched_barrier(0);
                    }
                    float sigma = wave_sum(Ps);  // wave-uniform: the rescaling below is a scalar branch
                    const uint32_t Sb = __builtin_amdgcn_readfirstlane(__float_as_uint(sigma));
                    if (Sb > 0x4f800000u && Sb < 0x7f800000u) {  // 2^32 < sigma < inf
                        uint32_t x = (Sb >> 23) - 127u;
                        x = x < 126u ? x : 126u;
                        const float down = __uint_as_float((127u - x) << 23);
#pragma unroll
                        for (int q = 0; q < S; ++q) {
                            M[q] *= down;
                            I[q] *= down;
                        }
                        bJ *= down;
                        bC *= down;
                        bN *= down;
                        sigma *= down;
                        e2 += static_cast<int32_t>(x);
                    }
                    // specials (row L: bC = move, the rest 0 -- sigma is 0 there, M and I being 0)
                    const float bB = sigma * a.tBM;
                    const float lJ = bJ * loop, lC = bC * loop, lN = bN * loop;
                    const float mB = move * bB;
                    bJ = lJ + mB;
                    bN = lN + mB;
                    bC = i == L ? move : lC;
                    const float bE = fmaf(bJ, a.tEJ, a.tEC * bC);
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

                    // D chain from the top, each lane's started from an incoming 0; g(k) = P(k+1)
                    const float gTop = shift1_down(M[0]);  // the right neighbour's first slot (0 into lane 63)
#pragma unroll
                    for (int c = C2 - 1; c >= 0; --c) {
                        const float2 tdm = tlds(B_DM, c), tdd = tlds(B_DD, c);
                        const float g1 = (c == C2 - 1) ? gTop : M[2 * c + 2];
                        const float u1 = fmaf(tdm.y, g1, bE);
                        D[2 * c + 1] = (c == C2 - 1) ? u1 : fmaf(tdd.y, D[2 * c + 2], u1);
                        // state 1 (lane 0, slot 0) is entered by no exit
                        const float x0 = (c == 0 && lane == 0) ? 0.0f : bE;
                        D[2 * c] = fmaf(tdd.x, D[2 * c + 1], fmaf(tdm.x, M[2 * c + 1], x0));
                        if constexpr (FENCE) __builtin_amdgcn_sched_barrier(0);
                    }
                    // the lanes' affine maps D_out = a D_in + b scanned inclusively towards lane 0: after step j,
                    // b is the lane's first D given an incoming 0 at lane l + 2^(j+1)
                    float b = D[0];
                    b = fmaf(A[0], shift1_down(b), b);
#pragma unroll
                    for (int j = 1; j < kScanSteps; ++j) b = fmaf(A[j], shift_down_by(b, lane, 1 << j), b);
                    const float Din = shift1_down(b);  // the exact D entering this lane from the right (0 into lane 63)
                    // fix-up, then bM and bI in place, lowest slot first: slot q reads P(q+1), not yet overwritten
#pragma unroll
                    for (int c = 0; c < C2; ++c) {
                        const float2 sf = tlds(B_SFX, c);
                        D[2 * c] = fmaf(Din, sf.x, D[2 * c]);
                        D[2 * c + 1] = fmaf(Din, sf.y, D[2 * c + 1]);
                        if constexpr (FENCE) __builtin_amdgcn_sched_barrier(0);
                    }
#pragma unroll
                    for (int c = 0; c < C2; ++c) {
                        const float2 tmm = tlds(B_MM, c), tmi = tlds(B_MI, c), tmd = tlds(B_MD, c);
                        const float2 tim = tlds(B_IM, c), tii = tlds(B_II, c);
                        const float g0 = M[2 * c + 1];
                        const float g1 = (c == C2 - 1) ? gTop : M[2 * c + 2];
                        const float d1 = (c == C2 - 1) ? Din : D[2 * c + 2];
                        const float h0 = I[2 * c], h1 = I[2 * c + 1];
                        M[2 * c] = fmaf(tmd.x, D[2 * c + 1], fmaf(tmi.x, h0, fmaf(tmm.x, g0, bE)));
                        I[2 * c] = fmaf(tii.x, h0, tim.x * g0);
                        M[2 * c + 1] = fmaf(tmd.y, d1, fmaf(tmi.y, h1, fmaf(tmm.y, g1, bE)));
                        I[2 * c + 1] = fmaf(tii.y, h1, tim.y * g1);
                        if constexpr (FENCE) __builtin_amdgcn_sched_barrier(0);
                    }
                }
                const float sc = fmaf(static_cast<float>(e2), 0.69314718055994529f, logf(bNout));
                if (lane == 0) a.scores[s] = sc;
            }
        }
        uint32_t t = 0;
        if (lane == 0) t = atomicAdd(a.counter, 1u);
        item = nwaves + __builtin_amdgcn_readfirstlane(t);
    }
    if (lane == 0) {
        __threadfence();
        if (atomicAdd(&exited_s, 1u) == WAVES - 1) seqq::count_leavers<1, 1>(a.counter);
    }
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
