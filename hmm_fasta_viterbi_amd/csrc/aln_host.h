// aln_host.h -- host-only half of the alignment stage (msv.h "Alignment stage"): the float64 posterior
// decoding of one envelope, THE definition of the optimal-accuracy (OA) alignment and its walk on float32 posterior
// arrays (the device kernels of aln_kernel.hip reproduce it bit for bit on the same arrays), the gate bytes those
// kernels read, and the workspace arithmetic.  No HIP include: aln_host.cpp is built by plain g++ and runs under the
// sanitizers (tests/cpp/sanitize_align.cpp).
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "fwd_host.h"
#include "msv.h"

namespace msv_host {

// The float64 decode of an envelope of Le residues (codes 0..19) whose loop / move are those of the configured
// length Lc: the envelope score log Z (nats) and, where the pointers are given, ppM / ppI as double [Le][M]
// (row i - 1, column k; column 0 and what the model has no state for stay 0) and ppN / ppJ / ppC as double [Le].
// Le = 0: score -inf, nothing written.
void aln_decode_on_envelope(const FwdModel& m, const uint8_t* codes, size_t Le, size_t Lc, double* score, double* ppM,
                            double* ppI, double* ppN, double* ppJ, double* ppC);

// The OA alignment of one envelope (msv.h states the recurrence and the tie-breaks): domains with seq = 0, i
// relative to the envelope (1 .. Le) and ops_begin from 0, one op byte and one posterior per core state visited.
struct AlnTrace {
    float score = 0.0f;  // C(Le); -inf where no path reaches C
    std::vector<msv_vit_domain> domains;
    std::vector<uint8_t> ops;
    std::vector<float> op_pp;
};
AlnTrace aln_oa_on_envelope(const float* ppM, const float* ppI, const float* ppN, const float* ppJ, const float* ppC,
                            const float* tsc, size_t M, float tr_B_Mk, float tr_E_C, float tr_E_J, size_t Le,
                            size_t Lc);

// The walk back from C(Le) over 4-bit cells and row records in vit_trace_plan.h's encoding: the ONE definition of
// the walk, which aln_oa_on_envelope and the device's walk kernel both run.  cell(i, k) gives the 4 bits of node k
// on row i, rec(i) the row's record; kmax bounds k (a corrupt workspace cannot lead outside it).  The path comes
// out backwards: op(c, i, k) once per core state visited, last first, then dom(i_from, i_to, k_from, k_to, len)
// once per domain, last first.  Every step lowers i or k, so the walk ends after at most Le + kmax steps a domain.
template <class Cell, class Rec, class Op, class Dom>
FWD_HD inline void aln_walk(uint64_t Le, uint32_t kmax, Cell cell, Rec rec, Op op, Dom dom) {
    constexpr uint32_t kFromM = 0, kFromI = 1, kFromB = 3, kIFromI = 4, kDFromD = 8;  // vit_trace_plan.h
    constexpr uint32_t kRecKMask = 0xffffu, kRecCFromE = 1u << 16, kRecJFromE = 1u << 17, kRecBFromJ = 1u << 18;
    uint64_t i = Le;
    while (i >= 1 && !(rec(i) & kRecCFromE)) --i;  // C loops
    while (i >= 1) {
        uint32_t k = rec(i) & kRecKMask;  // E(i) -> M(i, k)
        const uint32_t i_to = static_cast<uint32_t>(i), k_to = k;
        uint32_t i_from = 0, k_from = 0, len = 0;
        int st = 0;  // 0 M, 1 I, 2 D
        bool entered = false;
        while (!entered && i >= 1 && k >= 1 && k <= kmax) {
            const uint32_t b = cell(i, k);
            if (st == 0) {
                op('M', i, k);
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
                op('I', i, k);
                st = (b & kIFromI) ? 1 : 0;
                --i;
            } else {
                op('D', i, k);
                st = (b & kDFromD) ? 2 : 0;
                --k;
            }
            ++len;
        }
        dom(i_from, i_to, k_from, k_to, len);
        // B(i): from N (the path's start) or from J, which loops back to an earlier E
        if (!entered || i == 0 || !(rec(i) & kRecBFromJ)) break;
        while (i >= 1 && !(rec(i) & kRecJFromE)) --i;
    }
}

// Gate bits of a slot's byte (aln_kernel.hip's fill): which transitions INTO the slot's node k (and, for MI / II,
// out of its own M and I into its own I) are open, i.e. have a finite score, and whether B enters node k.
constexpr uint32_t kGateMM = 1, kGateIM = 2, kGateDM = 4, kGateMI = 8, kGateII = 16, kGateMD = 32, kGateDD = 64,
                   kGateBM = 128;
// The gate bytes of a variant of S states per lane, four slots a word: word w of lane l at [w * 64 + l], slot q in
// byte q % 4 of word q / 4 (padding slots and slots beyond LENG: 0).
std::vector<uint32_t> aln_gates(const float* tsc, uint32_t model_length, float tr_B_Mk, int S);

// Workspace of one item under a variant of S states per lane, all in 32-bit words: Le + 1 six-word special-state
// records (Forward's, then ppN / ppJ / ppC over the first three words of rows 1 .. Le), Le rows of 2 S x 64 floats
// (fM then fI by slot, then ppM / ppI in place), Le rows of ceil(S / 8) x 64 back-pointer words and Le row records.
constexpr uint64_t kAlnRowWords = 6;
constexpr uint64_t aln_pointer_words(uint64_t S) { return (S + 7) / 8; }
constexpr uint64_t aln_record_words(uint64_t Le) { return (Le + 1) * kAlnRowWords; }
constexpr uint64_t aln_matrix_words(uint64_t S, uint64_t Le) { return Le * 2 * S * 64; }
constexpr uint64_t aln_trace_words(uint64_t S, uint64_t Le) { return Le * (aln_pointer_words(S) * 64 + 1); }
constexpr uint64_t aln_item_bytes(uint64_t S, uint64_t Le) {
    return 4 * (aln_record_words(Le) + aln_matrix_words(S, Le) + aln_trace_words(S, Le));
}

}  // namespace msv_host
