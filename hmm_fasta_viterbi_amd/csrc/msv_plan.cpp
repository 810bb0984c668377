// msv_plan.cpp -- the MSV plan policy (msv_plan.h) and the measurements behind it.  No HIP.
#include "msv_plan.h"

#include <algorithm>

namespace msvplan {

// Estimated VALU of one row for one sequence: 2.5 per state-slot plus the per-row specials/reduction
// (G = 64: + permlane32 step, scalar bookkeeping), and for a split table the B-table address and loads.
double row_cost(const VariantShape& v) { return 2.5 * v.S + (v.G == 64 ? 36.0 : 26.0) + (v.sa ? 2.0 : 0.0); }

// Estimated issue cost of one row for one sequence: row_cost times the lanes a sequence occupies.  A BIG
// table costs little with one sequence per wave (G = 64: wave-uniform LDS/L2 row split) and a lot with 2-4
// sequences per wave (generic loads with per-lane address selects); measured on 2405.hmm: 7.4 vs 10.5 ms.
// A split table (the lane's last S - SA states read from L2 every row) costs the B-table address and
// loads per row and no class branch, so it also runs two sequences per wave (G = 32).
double variant_cost(const VariantShape& v) {
    // (G = 64 BIG: 1.15 -- 1901.hmm's 64 x 32 row-class plan measured 1.12 / 2.20 ms against 0.97 / 1.99 ms
    // for the 64 x 34 split plan at 3 / 2048 sequences, profiles/r02_latency_plans.jsonl)
    const double big = !v.big ? 1.0 : (v.G == 64 ? 1.15 : 1.6);
    return row_cost(v) * v.G * big * (v.pf == 2 ? 1.0 : 1.05) * (v.streams == 2 ? 1.15 : 1.0);
}

namespace {

// The cheapest entry of `all` covering `states` that satisfies `ok`, under `cost`; the first of equals.
template <class Shape, class Ok, class Cost>
int cheapest(const std::vector<Shape>& all, uint32_t states, Ok ok, Cost cost) {
    int best = -1;
    double best_cost = 0.0;
    for (int i = 0; i < static_cast<int>(all.size()); ++i) {
        if (static_cast<uint32_t>(all[i].states()) < states || !ok(all[i])) continue;
        const double c = cost(all[i]);
        if (best < 0 || c < best_cost) best = i, best_cost = c;
    }
    return best;
}

// A whole-row emission ring (PF = S/4: the next row's chunks requested during this row's epilogue) on
// 16 waves, for 16-lane rows of 16-32 states.
bool whole_row_ring(const VariantShape& v) {
    return v.G == 16 && v.streams == 1 && !v.big && !v.sa && v.pf * 4 == v.S && v.S >= 16 && v.S <= 32;
}

// `narrow`: 4-lane groups may be picked.  Their rows are long (16 sequences per wave), which the issue
// model rewards and which wins once the SIMDs are full, so they are the throughput plan of the smallest
// profiles (100.hmm x 100k: g4_s28 0.339 vs g16_s8 0.521 ms, x 1M 3.08 vs 4.11 ms) while batches that
// leave the SIMDs part-empty keep a 16-lane plan (x 10k: 0.138 vs 0.099 ms; choose).  8-lane
// groups stay tuning candidates: on 200.hmm g8_s32 against g16_s16 was 6% slower at 100k, 2% faster
// at 1M (profiles/r02_small_profiles.jsonl).
// `whole_row`: whole-row-ring variants are preferred where they exist -- on full batches 1-5% faster
// than the PF-2 ones (200/300/400/500.hmm x 100k: 0.692/0.827/1.051/1.196 vs 0.708/0.837/1.094/1.259 ms),
// while below a round of the grid the PF-2 ones hold (500.hmm x 10k: 0.229 vs 0.197 ms;
// profiles/r02_whole_row_rings.jsonl), so those stay the plan of smaller batches (choose).
int pick_variant(const Tables& t, uint32_t states, bool narrow, bool whole_row) {
    return cheapest(
        t.variants, states,
        // (not for tables of fewer than 80 states: a 28-state lane row would be mostly padding, unmeasured)
        [&](const VariantShape& v) { return v.G >= 16 || (narrow && v.G == 4 && states >= 80); },
        [&](const VariantShape& v) { return variant_cost(v) * (whole_row && whole_row_ring(v) ? 0.9 : 1.0); });
}

// Latency plan for small batches: one sequence per wave (G = 64) so a row is ~40% of the
// instructions of a 16-lane row; the cheapest such variant covering the model (non-BIG if any).
int pick_latency_variant(const Tables& t, uint32_t states) {
    return cheapest(t.variants, states, [](const VariantShape& v) { return v.G == 64; }, variant_cost);
}

// Mid plan for batches between the latency plan's and one round of the main grid: two sequences per
// wave (G = 32), the cheapest plain (LDS-table, one-stream) variant covering the model.
int pick_mid_variant(const Tables& t, uint32_t states) {
    return cheapest(
        t.variants, states, [](const VariantShape& v) { return v.G == 32 && v.streams == 1 && !v.big && !v.sa; },
        variant_cost);
}

// The smallest cooperative variant covering `states`, or -1.
int pick_coop_variant(const Tables& t, uint32_t states) {
    return cheapest(t.coop, states, [](const CoopShape&) { return true; }, [](const CoopShape& c) { return 1.0 * c.S; });
}

// Mid plan (G = 32, two sequences per wave) for G = 16 profiles with S >= 40 (~600-1536 states), taken
// by batches between the latency plan's range and about one round of the main grid.  There a 16-lane
// launch runs one partial round of 400-row sequences at ~2-3 waves per SIMD (latency-bound: ~4 ns per
// instruction per wave), and a 64-lane one needs 2-3 rounds; the 32-lane rows are half as long as the
// 16-lane ones at twice the waves.  1400.hmm x U[300,500]: 9000 sequences 0.388 ms against 0.458
// (latency plan) / 0.527 (main), 12000 0.464 vs 0.536 (main); 600.hmm x 6000 0.151 vs 0.245 (latency)
// / 0.175 (main); 900.hmm x 9000 0.299 vs 0.353 / 0.367 (profiles/r02_mid_plans.jsonl).
//  * upper end: 0.9 of one round of the main grid, and for S < 64 at most 10,752 sequences (3/4 of the
//    16,384 at which 16-lane launches fill 4 waves per SIMD: 800.hmm x 12000 ran 0.326 mid vs 0.291
//    main, while 1400.hmm x 12000 0.464 vs 0.536);
//  * lower end (the latency plan's new limit): where the 64-lane row stops being much shorter than the
//    32-lane one -- 15000 x (mid row / latency row - 1) sequences, within 1.5 rounds of the latency
//    grid: 1400.hmm (136 vs 96 VALU) ~6,100 (x 6000: 0.302 latency vs 0.306 mid), 600.hmm (76 vs 66)
//    2,270 (x 6000: mid 38% faster), 800.hmm (96 vs 76) 3,950 (x 6000: mid 8% faster).
// 500.hmm (S = 32) measured no consistent gain (the 32-lane plan won at some sizes and lost 10-15% at
// others) and keeps two plans.
void choose_mid(const Tables& t, uint32_t states, const BlocksOf& blocks_of, PlanSet& ps) {
    const int mv = pick_mid_variant(t, states);
    const VariantShape& main = t.variants[ps.main];
    if (mv < 0 || ps.lat < 0 || main.G != 16 || main.S < 40) return;
    const VariantShape& lat = t.variants[ps.lat];
    const uint64_t lat_cap = static_cast<uint64_t>(blocks_of(kLatency, ps.lat)) * lat.groups_per_block();
    const uint64_t main_cap = static_cast<uint64_t>(blocks_of(kMain, ps.main)) * main.groups_per_block();
    const double mid_row = row_cost(t.variants[mv]), lat_row = row_cost(lat);
    const uint64_t lat_by_rows = static_cast<uint64_t>(std::max(0.0, 15000.0 * (mid_row / lat_row - 1.0)));
    const uint64_t lat_max = std::min({ps.lat_max_n, lat_cap * 3 / 2, lat_by_rows});
    const uint64_t mid_max = std::min<uint64_t>(main_cap * 9 / 10, main.S >= 64 ? ~0ull : 10752);
    if (mid_max <= lat_max) return;
    ps.mid = mv;
    ps.lat_max_n = lat_max;
    ps.mid_max_n = mid_max;
}

// The cooperative plan (msv_coop.hip) for batches of at most one workgroup per CU: one sequence per
// workgroup, its row spread over 4 waves (one per SIMD) with halo states and a speculated B.  Chosen
// when a compiled CoopVariant covers the model (the whole table staged in LDS up to 1464 states, the
// split table -- each lane's last 2-4 states read from L2 -- up to 2480) and
// tr_E_C == tr_E_J (the reference's nu = 2, MSV_HMM.cpp:49-53), and never under a forced variant.
void choose_coop(const Tables& t, uint32_t states, const BlocksOf& blocks_of, PlanSet& ps) {
    ps.coop = pick_coop_variant(t, states);
    if (ps.coop < 0) return;
    // Up to where it beats the plan the batch would otherwise take (tools/coop_sweep.py,
    // profiles/r03_coop_sweep.jsonl; L U[300,500], kernel ms coop / other): 1400.hmm 512 seqs 0.106 /
    // 0.191, 1024 0.144 / 0.194, 2048 0.272 / 0.198; 1001.hmm 512 0.147 / 0.153; 1901.hmm 1024 0.243 /
    // 0.264; 2405.hmm (L ~2000) 1024 1.19 / 1.35; 400.hmm (S = 2, 768 workgroups) 512 0.037 / 0.105, 1024
    // 0.113 / 0.107; 100.hmm (no latency plan) 256 0.056 / 0.074, 512 0.071 / 0.074, 1024 0.099 / 0.074.
    // So two rounds of the grid for S >= 4, one for S = 2, half of one without a latency plan.
    const double rounds = (t.coop[ps.coop].S >= 4 ? 2.0 : 1.0) * (ps.lat >= 0 ? 1.0 : 0.5);
    ps.coop_max_n = static_cast<uint64_t>(rounds * blocks_of(kCoop, ps.coop));
}

}  // namespace

// Main plan (forced, or the cheapest with 4-lane groups and whole-row rings allowed); unless forced, the
// latency plan unless it would be the same kernel, a mid plan (choose_mid; or, when the main plan has 4-lane
// groups or a whole-row ring, the 16-lane PF-2 plan for batches that leave the SIMDs part-empty), and the
// cooperative plan in front of them (it needs to know whether a latency plan exists: choose_coop).
PlanSet choose(const Tables& t, uint32_t states, bool same_EJ, int forced_index, int cus, const BlocksOf& blocks_of) {
    PlanSet ps;
    const bool force = forced_index >= 0;
    ps.main = force ? forced_index : pick_variant(t, states, true, true);
    if (ps.main < 0) return ps;
    const VariantShape& main = t.variants[ps.main];
    // the 16+-lane plan the latency plan is weighed against, and the plan of batches below one round of
    // the grid: the main plan itself unless it is narrow (4 lanes) or a whole-row-ring variant
    const int v = (main.G < 16 || whole_row_ring(main)) && !force ? pick_variant(t, states, false, false) : ps.main;
    const int lv = force ? -1 : pick_latency_variant(t, states);
    // Worth it only when the 64-lane row is much shorter than the main row (per-row issue cost,
    // as variant_cost): 1400.hmm 246 vs 96 -> 0.23 vs 0.62 ms at 1024 sequences, 0.37 vs 0.64 at 8192,
    // even at 16384; 1901.hmm 176 vs 123 -> 0.97 vs 1.29 ms at 3 sequences, 1.99 vs 2.89 at 2048;
    // 100.hmm 46 vs 46 -> slower at every size (tools/tune.py, profiles/r01_latency_plan.jsonl,
    // r02_latency_plans.jsonl).
    // (The main row is weighed without a split table's + 2, as when the thresholds were measured.  A 64-lane
    // `v` never gets here: unforced it is itself the latency pick, lv == v.)
    const double main_row = row_cost(t.variants[v]) - (t.variants[v].sa ? 2.0 : 0.0);
    const double ratio = lv >= 0 ? main_row / row_cost(t.variants[lv]) : 0.0;
    if (v != ps.main) {
        // Narrow main plan: the 16-lane plan while it would not fill the SIMDs -- 3.5 of its waves per
        // SIMD, where a 16-lane launch turns issue-bound (100.hmm: 14,336 sequences on 256 CUs; the
        // crossover measured between 10k and 20k, profiles/r02_small_profiles.jsonl).  Whole-row-ring
        // main plan: the PF-2 variant up to 3/4 of that (10,752).
        const double fill = main.G < 16 ? 3.5 : 2.625;
        ps.mid = v;
        ps.mid_max_n = static_cast<uint64_t>(fill * 4 * cus * (64 / t.variants[v].G));
    }
    if (lv >= 0 && lv != v && ratio >= 1.3) {
        ps.lat = lv;
        ps.lat_max_n = static_cast<uint64_t>(std::min(12288.0, 4096.0 * ratio));
        if (ps.mid >= 0) ps.lat_max_n = std::min(ps.lat_max_n, ps.mid_max_n);
        else choose_mid(t, states, blocks_of, ps);
    }
    if (!force && same_EJ) choose_coop(t, states, blocks_of, ps);
    return ps;
}

// Latency (n <= lat_max_n), mid (n <= mid_max_n), else main, with the cooperative plan in front of them.
// Small batches take the latency plan: with fewer sequences than ~4 per SIMD the launch lasts one
// sequence's rows, and a 64-lane row is far shorter than a 16-lane one.  Mid-size ones (less than one round
// of the main grid) take the 32-lane plan where there is one (choose_mid).
Kind which(const PlanSet& ps, uint64_t n, bool latency_ok, bool host_residues) {
    if (!latency_ok) return kMain;
    // (not for residues read in place over PCIe: its 16-row residue blocks would wait on each one)
    if (ps.coop >= 0 && n <= ps.coop_max_n && !host_residues) return kCoop;
    if (ps.lat >= 0 && n <= ps.lat_max_n) return kLatency;
    if (ps.mid >= 0 && n <= ps.mid_max_n) return kMid;
    return kMain;
}

// A batch that takes the cooperative plan with at most one sequence per workgroup needs no dequeue order
// (every workgroup scores one sequence whatever the order): the host paths then skip the sort launch.
bool order_needless(const PlanSet& ps, uint64_t n, bool host_residues, int coop_blocks) {
    return which(ps, n, true, host_residues) == kCoop && n <= static_cast<uint64_t>(coop_blocks);
}

// A grid of few sequences (one 64-lane wave each, at most this many waves over all profiles) runs as ONE
// launch: every profile's batch takes the latency layout of the grid's largest model, so each
// profile's launch lasts about as long as it would alone, and all of them run at once instead of
// queueing on the process's hardware queues (4 by default: 24 profiles x 3 sequences of 3,500
// residues, benchmark_MSV's shape, took 4.05 ms as 24 launches).
constexpr uint64_t kFusedMaxSeqs = 2048;

// Fused in the cooperative layout: a grid of few sequences (n x profiles <= kFusedMaxSeqs), every profile
// with tr_E_C == tr_E_J and no forced variant, a variant covering the largest model -- and at most as many
// workgroups per launch (n x the launch's profiles) as the smallest coop_max_n of the listed profiles: the
// limit of the per-profile cooperative plan (about one workgroup fits a CU, so a launch of more is several
// rounds of the grid, and past ~2 rounds the cooperative plan loses).  coop_max_n = 0 (no
// cooperative plan, or msv_debug_set_coop_max_n(0)) turns the fused form off.  Residues read in place over
// PCIe (host_residues) keep the latency layout, as which() does.
// Else fused in the latency layout of the largest model, unless a profile is forced (msv_profile_set_variant:
// that variant for every batch) or a handle is listed more often than it has counter slots: a fused launch
// holds one slot per entry until it ends, so the handle would share a {next, waves left} pair between two
// sub-grids of one launch.
GridChoice fused_grid(const Tables& t, const GridProfile* profiles, uint32_t n_profiles, uint64_t n,
                      bool host_residues, uint32_t most_listed) {
    const GridChoice per_profile{GridChoice::kPerProfile, -1};
    if (n_profiles < 2 || n * n_profiles > kFusedMaxSeqs) return per_profile;
    uint32_t states = 0;
    bool forced = false, same_EJ = true;
    uint64_t cap = ~0ull;
    for (uint32_t i = 0; i < n_profiles; ++i) {
        states = std::max(states, profiles[i].states);
        forced |= profiles[i].forced;
        same_EJ &= profiles[i].same_EJ;
        cap = std::min(cap, profiles[i].coop_max_n);
    }
    if (!host_residues && !forced && same_EJ &&
        static_cast<uint64_t>(std::min(n_profiles, kGridMaxProfiles)) * n <= cap) {
        const int cv = pick_coop_variant(t, states);
        if (cv >= 0 && t.coop[cv].has_grid) return {GridChoice::kCoopFused, cv};
    }
    if (forced || most_listed > static_cast<uint32_t>(kLaunchSlots)) return per_profile;
    const int fv = pick_latency_variant(t, states);
    if (fv >= 0 && t.variants[fv].has_grid) return {GridChoice::kLatencyFused, fv};
    return per_profile;
}

// Each piece addresses < kChunkBytes residues and < 2^32 - 2^24 sequences (one launch each).  Batches below
// kPipelineMin residues are one piece; larger ones start at 1/first_den of the batch (at least 1M residues)
// and grow `growth`-fold, a short remainder joining the last piece.
std::vector<uint64_t> plan_pieces(const uint64_t* offsets, uint64_t n, uint64_t total, uint32_t first_den,
                                  uint32_t growth) {
    constexpr uint64_t kMaxSeqs = kMaxLaunchSeqs - 1;
    std::vector<uint64_t> cut{0};
    uint64_t want = (total < kPipelineMin || first_den == 0) ? kChunkBytes
                                                             : std::max<uint64_t>(1ull << 20, total / first_den);
    uint64_t first = 0;
    while (first < n) {
        const uint64_t base = offsets[first];
        auto end_of = [&](uint64_t budget) {  // last sequence index with offsets[last] - base <= budget
            const uint64_t* it = std::upper_bound(offsets + first + 1, offsets + n + 1, base + budget);
            return static_cast<uint64_t>(it - offsets) - 1;
        };
        uint64_t last = std::max(end_of(std::min(want, kChunkBytes - 1)), first + 1);  // >= one sequence
        last = std::min(last, first + kMaxSeqs);
        // a remainder shorter than this piece joins it (half the next piece at the default growth of 2),
        // if the chunk limit allows
        const uint64_t rest = offsets[n] - offsets[last];
        if (last < n && rest < want && offsets[n] - base < kChunkBytes && n - first <= kMaxSeqs) last = n;
        cut.push_back(last);
        first = last;
        want = std::min(kChunkBytes, std::max<uint32_t>(growth, 1) * want);
    }
    return cut;
}

void rebase_offsets(const uint64_t* offsets, uint64_t first, uint64_t last, uint64_t* out) {
    const uint64_t base = offsets[first];
    for (uint64_t i = first; i <= last; ++i) out[i - first] = offsets[i] - base;
}

bool in_place_wins(uint32_t states, uint64_t bytes) { return states >= kInPlaceMinStates || bytes < kInPlaceAnyBytes; }

CallPlan plan_call(const uint64_t* offsets, uint64_t n, uint64_t total, bool in_place, uint32_t first_den,
                   uint32_t growth) {
    CallPlan c;
    c.n = n;
    c.mode = in_place && total ? CallPlan::kInPlace
                               : (total <= kSmallCall && n <= kSmallCall ? CallPlan::kSmall : CallPlan::kCopied);
    c.cut = plan_pieces(offsets, n, total, c.mode == CallPlan::kInPlace ? 0 : first_den, growth);
    c.pipeline = c.mode == CallPlan::kCopied && c.pieces() > 1;
    c.res_words = c.mode == CallPlan::kSmall ? (total + 7) / 8 : 0;
    return c;
}

}  // namespace msvplan
