// table_layout.cpp -- the kernel-layout score tables, built on the host with no HIP in sight: pure index
// arithmetic over the residue-major host tables, so the sanitizer builds run it (tests/cpp/sanitize_host.cpp).
// msv_device.cpp and vit_device.cpp upload what these return.
#include <cstddef>
#include <cstdint>
#include <limits>
#include <vector>

#include "host_cpu.h"

namespace msv_host {

namespace {

// msv_kernel.h (msvk::) and vit_kernel.h (vitk::) name the same numbers; the device layer asserts that they agree.
constexpr int kAminoAcids = 20;
constexpr int kPoisonRow = 20;
constexpr int kTableRows = 21;
constexpr int kVitRows = 20;
constexpr int kVitTransitions = 7;
constexpr int kVitLanes = 64;
enum : int { MM_IN = 0, IM_IN = 1, DM_IN = 2, MI = 3, II = 4, MD_IN = 5, DD_IN = 6 };  // vitk:: slot arrays

constexpr float kNinf = -std::numeric_limits<float>::infinity();
constexpr float kPinf = std::numeric_limits<float>::infinity();

}  // namespace

// The MSV table of a variant with G lanes per sequence and S states per lane:
// [row r][chunk c][lane gl] float4 = e[r][gl*S + 4c + 1 .. +4]; states beyond LENG are -inf
// (never win a max); row 20 is the +inf poison row for codes >= 20.
// Split variants (sa > 0, G = 32/64, lane gl owns states gl*S + 1 .. gl*S + S as usual): an A table
// [20 rows][SA/4][G] float4 (the lane's first SA states, staged in LDS) followed by a B table
// [21 rows][G][HBP] float2 (its last S - SA states as HB = (S-SA)/2 halves padded to HBP = even,
// lane-contiguous so a lane reads them as HBP/2 float4 loads from L2; row 20 = poison).
std::vector<float> msv_variant_table(const float* es, uint32_t model_length, int G, int S, int sa) {
    const uint32_t R = model_length - 1;
    const int C4 = S / 4;
    const float ninf = kNinf, pinf = kPinf;
    std::vector<float> tab;
    // one [rows][chunks][G] block of `width`-float chunks whose lane gl, chunk c, slot q holds state
    // first + gl*span + width*c + q
    auto block = [&](int rows, int chunks, uint32_t first, int span, int width) {
        for (int r = 0; r < rows; ++r)
            for (int c = 0; c < chunks; ++c)
                for (int gl = 0; gl < G; ++gl)
                    for (int q = 0; q < width; ++q) {
                        const uint32_t j = first + static_cast<uint32_t>(gl * span + width * c + q);  // state 1..
                        float val;
                        if (r == kPoisonRow) val = pinf;
                        else val = (j <= R) ? es[static_cast<size_t>(r) * model_length + j] : ninf;
                        tab.push_back(val);
                    }
    };
    if (sa > 0) {
        block(kAminoAcids, sa / 4, 1, S, 4);
        // B table [21 rows][G][HBP] float2, lane-contiguous (each lane reads HBP/2 float4), HBP = the
        // lane's HB = (S - SA)/2 halves rounded up to even (the pad half is -inf and never read)
        const int HB = (S - sa) / 2, HBP = (HB + 1) & ~1;
        for (int r = 0; r < kTableRows; ++r)
            for (int gl = 0; gl < G; ++gl)
                for (int h = 0; h < HBP; ++h)
                    for (int q = 0; q < 2; ++q) {
                        const uint32_t j = static_cast<uint32_t>(sa + 1 + gl * S + 2 * h + q);  // state 1..
                        float val;
                        if (r == kPoisonRow) val = pinf;
                        else if (h < HB && j <= R) val = es[static_cast<size_t>(r) * model_length + j];
                        else val = ninf;
                        tab.push_back(val);
                    }
    } else {
        block(kTableRows, C4, 1, S, 4);
    }
    return tab;
}

// The lazy-E bound table of a whole-row variant (msv_kernel_body.inc, LAZY): [row r][lane gl] = the largest
// emission score of residue r over the lane's states gl*S + 1 .. gl*S + S.  States beyond LENG are
// ignored (a lane that holds only padding gets -inf); row 20, the poison row, is +inf, so a row with a
// bad residue never passes the bound.  It follows the variant's table in the same device buffer.
std::vector<float> msv_lazy_bound_table(const float* es, uint32_t model_length, int G, int S) {
    const uint32_t R = model_length - 1;
    std::vector<float> tab(static_cast<size_t>(kTableRows) * G, kPinf);
    for (int r = 0; r < kAminoAcids; ++r)
        for (int gl = 0; gl < G; ++gl) {
            float m = kNinf;
            for (int q = 0; q < S; ++q) {
                const uint32_t j = 1 + static_cast<uint32_t>(gl * S + q);  // state 1..
                if (j <= R && es[static_cast<size_t>(r) * model_length + j] > m)
                    m = es[static_cast<size_t>(r) * model_length + j];
            }
            tab[static_cast<size_t>(r) * G + gl] = m;
        }
    return tab;
}

// The MSV table of a cooperative variant (msv_coop.hip) of `waves` waves, S states per lane, the first sa of
// them staged in LDS, `halo` states shared between neighbouring waves:
// [21 rows][waves][SA/2 chunks][64 lanes] float2 (staged in LDS): wave w, lane l, chunk h, slot q holds
// global state w * (64 S - halo) - halo + l S + 2h + q + 1; split variants (SA < S) append
// [21 rows][waves][64 lanes][S - SA] floats for the lane's states SA .. S-1 (read from L2 per row).
// States outside 1..LENG are -inf; row 20 is the +inf poison row.
std::vector<float> msv_coop_table(const float* es, uint32_t model_length, int waves, int S, int sa, int halo) {
    const uint32_t R = model_length - 1;
    const int W = waves, SA = sa, H = SA / 2, SB = S - SA;
    const float ninf = kNinf, pinf = kPinf;
    auto value = [&](int r, int w, int l, int k) {
        const int64_t j = static_cast<int64_t>(w) * (64 * S - halo) - halo + l * S + k + 1;
        if (r == kPoisonRow) return pinf;
        return (j >= 1 && j <= R) ? es[static_cast<size_t>(r) * model_length + j] : ninf;
    };
    std::vector<float> tab;
    tab.reserve(static_cast<size_t>(kTableRows) * W * 64 * S);
    for (int r = 0; r < kTableRows; ++r)
        for (int w = 0; w < W; ++w)
            for (int h = 0; h < H; ++h)
                for (int l = 0; l < 64; ++l)
                    for (int q = 0; q < 2; ++q) tab.push_back(value(r, w, l, 2 * h + q));
    for (int r = 0; r < kTableRows && SB > 0; ++r)
        for (int w = 0; w < W; ++w)
            for (int l = 0; l < 64; ++l)
                for (int i = 0; i < SB; ++i) tab.push_back(value(r, w, l, SA + i));
    return tab;
}

// Kernel layouts of a Viterbi variant's tables (vit_kernel.h): slot q of (virtual) lane l is state k = l * S + q + 1;
// chunk c of a lane holds slots 2c, 2c + 1 as one float2, lanes contiguous (a team's 64 * team virtual lanes;
// an odd S leaves the last chunk's second slot unused).
VitTables vit_tables(const float* msc, const float* isc_tab, const float* tsc, uint32_t model_length, int S, int team,
                     bool isc) {
    const int C2 = (S + 1) / 2, L64 = kVitLanes * team;
    const uint32_t M = model_length, K = M - 1;
    const size_t row2 = static_cast<size_t>(C2) * L64;
    auto state = [&](int l, int q) -> uint32_t { return static_cast<uint32_t>(l * S + q + 1); };
    VitTables t;
    t.et.resize(2 * kVitRows * row2);
    t.it.resize(isc ? 2 * kVitRows * row2 : 0);
    t.tt.resize(2 * kVitTransitions * row2);
    for (int r = 0; r < kVitRows; ++r)
        for (int c = 0; c < C2; ++c)
            for (int l = 0; l < L64; ++l) {
                float e2[2], i2[2];
                for (int h = 0; h < 2; ++h) {
                    const uint32_t k = 2 * c + h < S ? state(l, 2 * c + h) : K + 1;  // (unused slot)
                    e2[h] = k <= K ? msc[static_cast<size_t>(r) * M + k] : kNinf;
                    i2[h] = (isc && k < K) ? isc_tab[static_cast<size_t>(r) * M + k] : 0.0f;
                }
                const size_t at = 2 * ((static_cast<size_t>(r) * C2 + c) * L64 + l);
                t.et[at] = e2[0], t.et[at + 1] = e2[1];
                if (isc) t.it[at] = i2[0], t.it[at + 1] = i2[1];
            }
    // per-slot transition arrays (vitk::MM_IN .. DD_IN); file order m->m m->i m->d i->m i->i d->m d->d
    enum { MM, MI_, MD, IM, II_, DM, DD };
    auto slot_t = [&](int j, uint32_t k) -> float {
        if (k > K) return kNinf;  // padding slots
        const float* tin = tsc + static_cast<size_t>(k - 1) * 7;  // node k-1 -> node k
        const float* tout = tsc + static_cast<size_t>(k) * 7;     // node k -> I(k)
        switch (j) {
            case MM_IN: return k >= 2 ? tin[MM] : kNinf;
            case IM_IN: return k >= 2 ? tin[IM] : kNinf;
            case DM_IN: return k >= 2 ? tin[DM] : kNinf;
            case MI: return k < K ? tout[MI_] : kNinf;
            case II: return k < K ? tout[II_] : kNinf;
            case MD_IN: return k >= 2 ? tin[MD] : kNinf;
            case DD_IN: return k >= 2 ? tin[DD] : kNinf;
        }
        return kNinf;
    };
    for (int j = 0; j < kVitTransitions; ++j)
        for (int c = 0; c < C2; ++c)
            for (int l = 0; l < L64; ++l) {
                const size_t at = 2 * ((static_cast<size_t>(j) * C2 + c) * L64 + l);
                t.tt[at] = slot_t(j, state(l, 2 * c));
                t.tt[at + 1] = slot_t(j, 2 * c + 1 < S ? state(l, 2 * c + 1) : K + 1);
            }
    return t;
}

}  // namespace msv_host
