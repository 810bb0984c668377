// spl_host.h -- host-only half of the split stage (msv.h "Split stage"): THE definition of one
// stochastic traceback sample (the walk, the draw and the random numbers, which spl_kernel.hip's sampler runs too and
// reproduces byte for byte on the same arrays), the float64 Forward twin with D, the clustering and the workspace
// arithmetic.  No HIP include: spl_host.cpp is built by plain g++ and runs under the sanitizers
// (tests/cpp/sanitize_split.cpp).
//
// Floating point: every weight is one float32 product and every sum adds rounded terms, so no multiply may be fused
// into an add.  The device objects are built with -ffp-contract=off (DEVFLAGS); the host object of this header,
// spl_host.o, is too (the Makefile says so).
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "fwd_host.h"
#include "msv.h"

namespace msv_host {

// ---- random numbers: counter-based, stateless, integers only (msv.h states the mix)
FWD_HD inline uint64_t spl_mix(uint64_t x) {
    x ^= x >> 30;
    x *= 0xbf58476d1ce4e5b9ull;
    x ^= x >> 27;
    x *= 0x94d049bb133111ebull;
    x ^= x >> 31;
    return x;
}
constexpr uint64_t kSplGolden = 0x9e3779b97f4a7c15ull;
// The key of a sample: the envelope's identity, not its place in any list.
FWD_HD inline uint64_t spl_key(uint64_t seed, uint32_t seq, uint32_t i_from, uint32_t i_to, uint32_t sample) {
    uint64_t h = seed;
    h = spl_mix(h + kSplGolden + seq);
    h = spl_mix(h + kSplGolden + i_from);
    h = spl_mix(h + kSplGolden + i_to);
    h = spl_mix(h + kSplGolden + sample);
    return h;
}
// Draw d of the sample: 24 bits.
FWD_HD inline uint32_t spl_rand24(uint64_t key, uint32_t d) {
    return static_cast<uint32_t>(spl_mix(key + kSplGolden * (static_cast<uint64_t>(d) + 1)) >> 40);
}

// x 2^-down by multiplications by exact powers of two (each correctly rounded on the host and on the device alike;
// exact while the result is a normal number).  The recording kernel's exponents never fall from a row to the next,
// so the sampler calls it with down >= 0; a negative down (arrays of another origin) is the same move upward.
FWD_HD inline float spl_scale_down(float x, int32_t down) {
    while (down > 64) {
        x *= 0x1p-64f;
        down -= 64;
    }
    while (down < -64) {
        x *= 0x1p64f;
        down += 64;
    }
    union {
        uint32_t u;
        float f;
    } p;
    p.u = static_cast<uint32_t>(127 - down) << 23;  // 2^-down, -64 <= down <= 64
    return x * p.f;
}

// One draw among n weights (msv.h): the index, or -1 where T = 0.
template <int N>
FWD_HD inline int spl_draw(const float (&w)[N], uint32_t u24) {
    float T = w[0];
    for (int j = 1; j < N; ++j) T = T + w[j];
    if (!(T > 0.0f)) return -1;
    const float t = (static_cast<float>(u24) * 0x1p-24f) * T;
    float run = 0.0f;
    int last = -1;
    for (int j = 0; j < N; ++j) {
        run = run + w[j];
        if (w[j] > 0.0f) {
            if (run > t) return j;
            last = j;
        }
    }
    return last;
}

// The float32 odds the sampler multiplies by: tr [M][7] = (float) exp((double) score) of the transitions out of
// nodes 1 .. LENG-1 (0 elsewhere) -- the values spl_odds builds, the same expression that fills the device's slot
// arrays (fwd_host.cpp's fwd_tables) -- and the specials' odds as the domain profile holds them.
struct SplOdds {
    const float* tr;
    float tBM, tEC, tEJ, loop;
};
std::vector<float> spl_odds(const float* tsc, uint32_t model_length);
float spl_odds_of(float score);

// THE walk of one sample back from C(Le) over the recorded planes.  cell(plane, i, k): plane 0 fM, 1 fI, 2 fD of
// row i in 1 .. Le and node k in 1 .. LENG, in the scale of row i; rec(i, w): word w of row i's record, i in
// 0 .. Le (0 N, 1 J, 2 C, 3 B, 4 E as float bits, 5 the exponent).  The path comes out backwards as aln_walk's
// does: op(c, i, k) once per core state, last first, then dom(i_from, i_to, k_from, k_to, len) once per domain,
// last first.  Returns false where a draw met T = 0 (the sample is truncated; the domain under way is not
// reported).  Every step lowers i or k.
template <class Cell, class Rec, class Op, class Dom>
FWD_HD inline bool spl_sample(uint64_t Le, uint32_t LENG, Cell cell, Rec rec, const SplOdds& o, uint64_t key, Op op,
                              Dom dom) {
    enum { MM, MI, MD, IM, II, DM, DD };  // file order m->m m->i m->d i->m i->i d->m d->d
    union FU {
        uint32_t u;
        float f;
    };
    auto special = [&](uint64_t i, int w) -> float {
        FU x;
        x.u = rec(i, w);
        return x.f;
    };
    auto expo = [&](uint64_t i) -> int32_t { return static_cast<int32_t>(rec(i, 5)); };
    uint32_t d = 0;
    // a looping special X (1 J, 2 C) at row i >= 1: X(i-1) loop in row i's scale | E(i) tEX
    auto loop_or_e = [&](uint64_t i, int which, float tE) -> int {
        const float older = spl_scale_down(special(i - 1, which), expo(i) - expo(i - 1));
        const float w[2] = {older * o.loop, special(i, 4) * tE};
        return spl_draw(w, spl_rand24(key, d++));
    };
    uint64_t i = Le;
    int pick;
    if (i == 0) return true;
    while ((pick = loop_or_e(i, 2, o.tEC)) == 0) {  // C loops
        if (--i == 0) return false;                 // (C(0) = 0: never picked while T > 0)
    }
    if (pick < 0) return false;
    for (;;) {
        // E(i): two passes over the row
        uint32_t k = 0;
        int st = 0;  // 0 M, 1 I, 2 D
        {
            float T = cell(0, i, 1);
            for (uint32_t c = 2; c <= LENG; ++c) {
                T = T + cell(0, i, c);
                T = T + cell(2, i, c);
            }
            if (!(T > 0.0f)) return false;
            const float t = (static_cast<float>(spl_rand24(key, d++)) * 0x1p-24f) * T;
            float run = 0.0f;
            uint32_t last_k = 0;
            int last_st = 0;
            for (uint32_t c = 1; c <= LENG && k == 0; ++c) {
                for (int s = 0; s <= (c >= 2 ? 2 : 0); s += 2) {
                    const float w = cell(s, i, c);
                    run = run + w;
                    if (w > 0.0f) {
                        last_k = c;
                        last_st = s;
                        if (run > t) {
                            k = c;
                            st = s;
                            break;
                        }
                    }
                }
            }
            if (k == 0) {
                k = last_k;
                st = last_st;
            }
        }
        const uint32_t i_to = static_cast<uint32_t>(i), k_to = k;
        uint32_t i_from = 0, k_from = 0, len = 0;
        bool entered = false;
        while (!entered) {
            if (st == 0) {
                op('M', i, k);
                const bool core = i >= 2 && k >= 2;  // row 0 and node 0 hold zeros
                const float* t = o.tr + static_cast<size_t>(k - 1) * 7;
                const float w[4] = {core ? cell(0, i - 1, k - 1) * t[MM] : 0.0f,
                                    core ? cell(1, i - 1, k - 1) * t[IM] : 0.0f,
                                    core ? cell(2, i - 1, k - 1) * t[DM] : 0.0f, special(i - 1, 3) * o.tBM};
                const int src = spl_draw(w, spl_rand24(key, d++));
                if (src < 0) return false;
                if (src == 3) {
                    entered = true;
                    i_from = static_cast<uint32_t>(i);
                    k_from = k;
                } else {
                    st = src;
                }
                --i;
                --k;
            } else if (st == 1) {
                op('I', i, k);
                const bool core = i >= 2;
                const float* t = o.tr + static_cast<size_t>(k) * 7;
                const float w[2] = {core ? cell(0, i - 1, k) * t[MI] : 0.0f, core ? cell(1, i - 1, k) * t[II] : 0.0f};
                const int src = spl_draw(w, spl_rand24(key, d++));
                if (src < 0) return false;
                st = src;
                --i;
            } else {
                op('D', i, k);
                const bool core = k >= 2;
                const float* t = o.tr + static_cast<size_t>(core ? k - 1 : 0) * 7;
                const float w[2] = {core ? cell(0, i, k - 1) * t[MD] : 0.0f, core ? cell(2, i, k - 1) * t[DD] : 0.0f};
                const int src = spl_draw(w, spl_rand24(key, d++));
                if (src < 0) return false;
                st = src == 0 ? 0 : 2;
                --k;
            }
            ++len;
        }
        dom(i_from, i_to, k_from, k_to, len);
        // B(i): from N (the path's start) or from J, which loops back to an earlier E
        {
            const float w[2] = {special(i, 0), special(i, 1)};
            const int src = spl_draw(w, spl_rand24(key, d++));
            if (src < 0) return false;
            if (src == 0) return true;
        }
        if (i == 0) return false;  // (J(0) = 0)
        while ((pick = loop_or_e(i, 1, o.tEJ)) == 0) {
            if (--i == 0) return false;
        }
        if (pick < 0) return false;
    }
}

// One sample on arrays laid out as msv_spl_result_matrix returns them.
struct SplSample {
    bool truncated = false;
    std::vector<msv_spl_segment> segments;  // residues relative to the envelope, in residue order
    std::vector<msv_vit_domain> domains;
    std::vector<uint8_t> ops;
};
SplSample spl_sample_on_arrays(const float* fM, const float* fI, const float* fD, const uint32_t* records, size_t Le,
                               size_t M, const SplOdds& o, uint64_t key);

// The float64 twin of the recording launch (msv.h, msv_spl_cpu_forward); outputs may be null.
void spl_forward_on_envelope(const FwdModel& m, const uint8_t* codes, size_t Le, size_t Lc, double* score, double* fM,
                             double* fI, double* fD, double* specials, int32_t* exponents);

bool dom_is_multidomain(const float* begin, const float* end, uint32_t i_from, uint32_t i_to, float rt3);

struct SplClusterRule {
    uint32_t ov_num = 4, ov_den = 5, max_diagdiff = 4, post_num = 1, post_den = 4, end_num = 1, end_den = 50;
};
std::vector<msv_spl_envelope> spl_cluster(const msv_spl_segment* seg, size_t n, uint32_t n_samples,
                                          const SplClusterRule& rule);

// Workspace of one item under a variant of S states per lane, in 32-bit words: Le + 1 six-word records, then Le
// rows of 3 S x 64 floats: fM, fI, fD by slot, [row][plane * S + slot][lane].
constexpr uint64_t spl_record_words(uint64_t Le) { return (Le + 1) * 6; }
constexpr uint64_t spl_matrix_words(uint64_t S, uint64_t Le) { return Le * 3 * S * 64; }
constexpr uint64_t spl_item_bytes(uint64_t S, uint64_t Le) {
    return 4 * (spl_record_words(Le) + spl_matrix_words(S, Le));
}

}  // namespace msv_host
