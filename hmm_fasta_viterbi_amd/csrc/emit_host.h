// emit_host.h -- host-only half of the emit stage (msv.h "Emit stage"): THE definition of one emitted
// sequence (the walk, its keys and its draws, which emit.hip's count and place kernels run too and reproduce byte for
// byte), the integer tables and the score of a true path.  Integers only on the walk: no floating point is compiled
// into it, so the bytes cannot depend on the compiler.  No HIP include: emit_host.cpp is built by plain g++ and runs
// under the sanitizers (tests/cpp/sanitize_emit.cpp).
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "fwd_host.h"
#include "msv.h"
#include "spl_host.h"  // spl_mix, kSplGolden: the split stage's random numbers, unchanged

namespace msv_host {

constexpr int kEmitThresholds = 19;
constexpr uint64_t kEmitDefaultLength = 400;
constexpr uint64_t kEmitDefaultMaxLength = 1ull << 20;
constexpr uint64_t kEmitDefaultWorkspace = 256ull << 20;
constexpr uint32_t kEmitMaxLeng = 65535;  // LENG (LENG + 1) / 2 < 2^31
constexpr uint64_t kEmitMaxResidues = (1ull << 32) - (1ull << 20);  // of one device call: the engines' kChunkBytes

// The key of sequence s: chained as cal_key chains its fields, under a tag no sample set of calibration has.
FWD_HD inline uint64_t emit_key(uint64_t seed, uint64_t s) {
    uint64_t h = seed;
    h = spl_mix(h + kSplGolden + MSV_EMIT_STREAM);
    h = spl_mix(h + kSplGolden + s);
    return h;
}
// Draw d of the walk: one more mix, as spl_rand24 (d is 64 bits here: a walk may make more than 2^32 draws).
FWD_HD inline uint64_t emit_draw(uint64_t key, uint64_t d) { return spl_mix(key + kSplGolden * (d + 1)); }
FWD_HD inline uint32_t emit_rand24(uint64_t key, uint64_t d) { return static_cast<uint32_t>(emit_draw(key, d) >> 40); }
FWD_HD inline uint32_t emit_rand32(uint64_t key, uint64_t d) { return static_cast<uint32_t>(emit_draw(key, d) >> 32); }

// The count rule over a row of 19 thresholds: the residue code of one 24-bit draw.
FWD_HD inline uint32_t emit_code(const uint32_t* T, uint32_t u) {
    uint32_t c = 0;
    for (int j = 0; j < kEmitThresholds; ++j) c += u >= T[j] ? 1u : 0u;
    return c;
}

// Pairs (k_start, k_end) before k_start = s, s in 1 .. LENG + 1.
FWD_HD inline uint64_t emit_pairs_before(uint64_t s, uint64_t leng) { return (s - 1) * leng - (s - 1) * (s - 2) / 2; }
// The fragment of pair index idx < LENG (LENG + 1) / 2: the largest s with emit_pairs_before(s) <= idx.
FWD_HD inline void emit_fragment(uint32_t idx, uint32_t leng, uint32_t* k_start, uint32_t* k_end) {
    uint32_t lo = 1, hi = leng;  // the answer lies in [lo, hi]
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        if (emit_pairs_before(mid, leng) <= idx) lo = mid;
        else hi = mid - 1;
    }
    *k_start = lo;
    *k_end = lo + (idx - static_cast<uint32_t>(emit_pairs_before(lo, leng)));
}

// What the walk reads that is not a table row: by value into the kernels.
struct EmitConfig {
    uint32_t bg[kEmitThresholds];
    uint32_t t_loop, t_j;  // u < t_loop loops; u < t_j takes J (0 for unihit: no draw is made)
    uint32_t leng, max_length;  // max_length >= 1
    uint32_t multihit, file_inserts;  // (the insert rows hold the background's thresholds where file_inserts is 0)
};
struct EmitCounts {
    uint32_t length, domains, ops, truncated;
};

// THE walk of sequence `key`.  match / insert: rows of 19 thresholds, row k at [k * 19] (the insert rows of nodes
// 1 .. LENG-1 repeat the background's under MSV_INSERTS_ZERO, so the walk reads one table either way); trans: 4 words
// per node (T_MM, T_MM+MI, T_IM, T_DM).  The sink takes residue(code) once per residue in sequence order, op(c) once
// per core state in path order and domain(i_from, i_to, k_from, k_to, ops_len) when a domain closes; a counting sink
// ignores them all, a placing sink stores them, and both get the same counters back.
template <class Sink>
FWD_HD inline EmitCounts emit_walk(const EmitConfig& c, const uint32_t* match, const uint32_t* insert,
                                   const uint32_t* trans, uint64_t key, Sink& sink) {
    EmitCounts n = {0, 0, 0, 0};
    uint64_t d = 0;
    // a looping special: background residues while a draw says loop; false where max_length ended the walk
    auto flank = [&]() -> bool {
        while (emit_rand24(key, d++) < c.t_loop) {
            sink.residue(emit_code(c.bg, emit_rand24(key, d++)));
            if (++n.length == c.max_length) return false;
        }
        return true;
    };
    if (!flank()) {
        n.truncated = 1;
        return n;
    }
    const uint32_t npairs = c.leng * (c.leng + 1) / 2;
    for (;;) {
        uint32_t k, k_end;
        emit_fragment(static_cast<uint32_t>((static_cast<uint64_t>(emit_rand32(key, d++)) * npairs) >> 32), c.leng, &k,
                      &k_end);
        const uint32_t k_from = k, i_from = n.length + 1;
        uint32_t len = 0;
        int st = 0;  // 0 M, 1 I, 2 D
        bool full = false;
        for (;;) {
            if (st == 0) {
                sink.op('M');
                ++len;
                sink.residue(emit_code(match + static_cast<size_t>(k) * kEmitThresholds, emit_rand24(key, d++)));
                if (++n.length == c.max_length) {
                    full = true;
                    break;
                }
                if (k == k_end) break;
                const uint32_t u = emit_rand24(key, d++);
                const uint32_t* t = trans + static_cast<size_t>(k) * 4;
                const uint32_t pick = (u >= t[0] ? 1u : 0u) + (u >= t[1] ? 1u : 0u);
                if (pick == 1) {
                    st = 1;
                } else {
                    st = pick == 0 ? 0 : 2;
                    ++k;
                }
            } else if (st == 1) {
                sink.op('I');
                ++len;
                sink.residue(emit_code(insert + static_cast<size_t>(k) * kEmitThresholds, emit_rand24(key, d++)));
                if (++n.length == c.max_length) {
                    full = true;
                    break;
                }
                if (emit_rand24(key, d++) < trans[static_cast<size_t>(k) * 4 + 2]) {
                    st = 0;
                    ++k;
                }
            } else {
                sink.op('D');
                ++len;
                if (k == k_end) break;
                st = emit_rand24(key, d++) < trans[static_cast<size_t>(k) * 4 + 3] ? 0 : 2;
                ++k;
            }
        }
        sink.domain(i_from, n.length, k_from, k, len);
        n.domains += 1;
        n.ops += len;
        if (full) {
            n.truncated = 1;
            return n;
        }
        const bool again = c.multihit && emit_rand24(key, d++) < c.t_j;
        if (!flank()) {  // J or C
            n.truncated = 1;
            return n;
        }
        if (!again) return n;
    }
}

struct EmitCountSink {
    FWD_HD void residue(uint32_t) {}
    FWD_HD void op(uint32_t) {}
    FWD_HD void domain(uint32_t, uint32_t, uint32_t, uint32_t, uint32_t) {}
};
// Stores into arrays at this sequence's offsets; domains and ops may be null (no truth).
struct EmitPlaceSink {
    uint8_t* codes;
    msv_vit_domain* domains;
    uint8_t* ops;
    uint32_t seq;
    uint64_t ops_begin;
    FWD_HD void residue(uint32_t code) { *codes++ = static_cast<uint8_t>(code); }
    FWD_HD void op(uint32_t c) {
        if (ops) *ops++ = static_cast<uint8_t>(c);
    }
    FWD_HD void domain(uint32_t i_from, uint32_t i_to, uint32_t k_from, uint32_t k_to, uint32_t len) {
        if (domains) {
            msv_vit_domain r;
            r.seq = seq;
            r.i_from = i_from;
            r.i_to = i_to;
            r.k_from = k_from;
            r.k_to = k_to;
            r.ops_len = len;
            r.ops_begin = ops_begin;
            *domains++ = r;
        }
        ops_begin += len;
    }
};

// The tables of a profile under a configuration; status MSV_ERR_INVALID_ARGUMENT where a group has no total.
struct EmitTables {
    EmitConfig config;
    uint32_t model_length = 0;
    uint64_t length = 0;
    std::vector<uint32_t> match, insert, trans;  // [M][19], [M][19], [M][4]
    uint64_t bytes() const { return 4 * (match.size() + insert.size() + trans.size()); }
};
msv_status emit_tables(const msv_hmm* hmm, const msv_emit_options* options, EmitTables* out);

// Device bytes of a chunk (msv.h, msv_emit_workspace_bytes) and its parts, each rounded up to 16 bytes.
constexpr uint64_t emit_round16(uint64_t b) { return (b + 15) / 16 * 16; }
constexpr uint64_t emit_fixed_bytes(uint64_t n, bool truth) {
    return 16 * n + emit_round16(8 * (n + 1)) + (truth ? emit_round16(8 * (n + 1)) + emit_round16(n) : 0);
}
constexpr uint64_t emit_workspace_bytes(uint64_t n, uint64_t residues, uint64_t domains, uint64_t ops, bool truth) {
    return emit_fixed_bytes(n, truth) + emit_round16(residues) +
           (truth ? emit_round16(domains * sizeof(msv_vit_domain)) + emit_round16(ops) : 0);
}

}  // namespace msv_host

// The result object of msv_emit_generate and msv_emit_batch.
struct msv_emit_result {
    std::vector<uint8_t> codes, ops, truncated;
    std::vector<uint64_t> offsets, domain_offsets;
    std::vector<msv_vit_domain> domains;
    uint64_t chunks = 0;
    bool truth = true;
};
