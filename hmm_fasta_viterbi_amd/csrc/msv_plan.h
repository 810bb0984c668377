// msv_plan.h -- the MSV plan policy, host-only: which kernel variants a profile gets and up to how many
// sequences each is taken, which of them a batch takes, whether a grid of profiles runs as one fused launch,
// how a host batch is cut into pipeline pieces, and how a host call stages it (mode, layout of its one offsets
// upload, rebased offsets).  Pure arithmetic over the shapes of the compiled variants
// (msv_plan.cpp has the measurements behind it): no HIP header, so tests/cpp/sanitize_host.cpp runs it on the
// CPU against the plans recorded on the device (tests/golden/msv_plans.json).  msv_device.cpp installs what
// it says.
#pragma once

#include <cstdint>
#include <functional>
#include <vector>

namespace msvplan {

// Every launch addresses < 2^32 residue bytes and fewer than kMaxLaunchSeqs sequences.
constexpr uint64_t kChunkBytes = (1ull << 32) - (1ull << 20);
constexpr uint64_t kMaxLaunchSeqs = (1ull << 32) - (1ull << 24);
// Host batches of at least this many residues are scored as a copy/compute pipeline of pieces.
constexpr uint64_t kPipelineMin = 4ull << 20;
// Dequeue-counter slots of one profile (launch_ring.h); profiles of one fused launch (msv_kernel.h).
constexpr int kLaunchSlots = 8;
constexpr uint32_t kGridMaxProfiles = 32;

// The shape of entry i of msvk::variants() / msvk::coop_variants(), at index i; the order of the tables is the
// tie-break of every pick (gen_variants.py).
struct VariantShape {
    int G, S, waves, pf, streams, sa;
    bool big, has_grid;
    int states() const { return G * S; }
    int groups_per_block() const { return waves * (64 / G) * streams; }
};
struct CoopShape {
    int waves, S, halo, sa;
    bool has_grid;
    int states() const { return waves * (64 * S - halo); }
};
struct Tables {
    std::vector<VariantShape> variants;
    std::vector<CoopShape> coop;
};

enum Kind { kMain, kLatency, kMid, kCoop };

// The plans of one profile: table indices (-1: none) and the largest batch each small-batch plan takes.
struct PlanSet {
    int main = -1, lat = -1, mid = -1, coop = -1;
    uint64_t lat_max_n = 0;   // batches up to this many sequences take the latency plan
    uint64_t mid_max_n = 0;   // batches above lat_max_n and up to this many take the mid plan
    uint64_t coop_max_n = 0;  // batches up to this many sequences take the cooperative plan
};

double row_cost(const VariantShape& v);
double variant_cost(const VariantShape& v);

// The persistent grid size of entry `index` of the variant table (kMain, kLatency) or of the cooperative
// table (kCoop); choose() asks for no other kind.
using BlocksOf = std::function<int(Kind kind, int index)>;

// The plans of a model of `states` match states.  same_EJ: tr_E_C == tr_E_J bitwise; forced_index: the variant
// msv_profile_set_variant named, or -1; cus: the device's compute units.  main = -1: no variant covers it.
PlanSet choose(const Tables& t, uint32_t states, bool same_EJ, int forced_index, int cus, const BlocksOf& blocks_of);

// The plan a launch of n sequences takes.  latency_ok: it may take a small-batch plan; host_residues: the
// residues are read in place over PCIe.
Kind which(const PlanSet& ps, uint64_t n, bool latency_ok, bool host_residues);
// Whether the batch needs no dequeue order (coop_blocks: the cooperative plan's grid).
bool order_needless(const PlanSet& ps, uint64_t n, bool host_residues, int coop_blocks);

// How a grid of n sequences x the listed profiles runs: fused in the cooperative layout coop[index], fused in
// the latency layout variants[index], or a launch per profile.  most_listed: the most times one handle is listed.
struct GridProfile {
    uint32_t states;
    bool forced, same_EJ;
    uint64_t coop_max_n;
};
struct GridChoice {
    enum { kPerProfile, kCoopFused, kLatencyFused } kind;
    int index;
};
GridChoice fused_grid(const Tables& t, const GridProfile* profiles, uint32_t n_profiles, uint64_t n,
                      bool host_residues, uint32_t most_listed);

// Pieces of a host batch for msv_score_batch's copy/compute pipeline: cut[k] .. cut[k+1] is piece k's
// sequence range.
std::vector<uint64_t> plan_pieces(const uint64_t* offsets, uint64_t n, uint64_t total, uint32_t first_den,
                                  uint32_t growth);

// Writes sequences [first, last) of a CSR as a batch of its own: out[i] = offsets[first + i] - offsets[first]
// for i = 0 .. last - first (last - first + 1 words).  Every host path rebases through this.
void rebase_offsets(const uint64_t* offsets, uint64_t first, uint64_t last, uint64_t* out);

// Small host calls (pageable residues of at most kSmallCall bytes, at most kSmallCall sequences -- the
// reference's one-sequence-per-call pattern): residues staged behind the offsets in the pinned offsets
// buffer and sent in ONE H2D; pageable scores written by the kernel into pinned staging (no D2H).
constexpr uint64_t kSmallCall = 1ull << 20;
// Page-locked residues are read in place unless the model has fewer than kInPlaceMinStates states and the
// batch at least kInPlaceAnyBytes residues (the measurements: msv_device.cpp msv_score_batch).
constexpr uint32_t kInPlaceMinStates = 300;
constexpr uint64_t kInPlaceAnyBytes = 16ull << 20;
bool in_place_wins(uint32_t states, uint64_t bytes);

// What msv_score_batch decides before it enqueues anything: how the residues reach the kernels, the pieces, and
// the layout of the call's staging words (uint64): words [0, upload_words()) go to the device in one H2D, the
// pinned host buffer has the error word behind them.
struct CallPlan {
    // in place: page-locked residues read where they are; small: residues behind the offsets in their H2D (one
    // piece); copied: residues copied to the device, piece by piece under the kernels when `pipeline`
    enum Mode { kInPlace, kSmall, kCopied } mode = kCopied;
    bool pipeline = false;      // kCopied in several pieces: a copy stream and alternating compute streams
    uint64_t n = 0;             // sequences
    std::vector<uint64_t> cut;  // piece k = sequences cut[k] .. cut[k + 1] (plan_pieces)
    uint64_t res_words = 0;     // kSmall: the residues' words
    size_t pieces() const { return cut.size() - 1; }
    uint64_t offsets_word(size_t k) const { return cut[k] + k; }  // piece k's rebased offsets: up to cut[k + 1] + k
    uint64_t small_res_word() const { return n + pieces(); }
    uint64_t upload_words() const { return n + pieces() + res_words; }
    uint64_t err_word() const { return upload_words(); }  // host only: the call's error bits come back here
    uint64_t staged_words() const { return upload_words() + 1; }
};
// in_place: the residues are page-locked, zero-copy is on and in_place_wins (never a batch without residues).
// first_den, growth: plan_pieces' for a copied call; one read in place is cut at the launch limits only.
CallPlan plan_call(const uint64_t* offsets, uint64_t n, uint64_t total, bool in_place, uint32_t first_den,
                   uint32_t growth);

}  // namespace msvplan
