// sanitize_item_plan.cpp -- the chunked host calls' plan under AddressSanitizer / UBSan (csrc/Makefile `asan_items`):
// item_plan.h's chunk layout and item batch against a per-item restatement written here, on seeded random cases and
// on the edges named below.  Host-only sources, its own main.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "item_plan.h"
#include "msv.h"

#define REQUIRE(cond)                                                        \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                    \
        }                                                                    \
    } while (0)

namespace {

using itemplan::ChunkLayout;
using itemplan::ItemBatch;

constexpr msv_status kBad = MSV_ERR_INVALID_ARGUMENT;

uint64_t bytes_of(uint64_t Le) { return 4 * (3 * Le + 2); }  // a record per row and a head, in words

// The restatement: entry after entry, a new chunk where the entry does not fit any more or the chunk is full.
struct Naive {
    bool ok = true;
    std::vector<uint64_t> chunk_of, base;
    std::vector<uint64_t> first;  // per chunk
    uint64_t most_units = 0, most_entries = 0, total_units = 0;
};
Naive naive_layout(const std::vector<uint64_t>& bytes, uint64_t budget, uint64_t unit, uint64_t cap) {
    Naive v;
    // the cap cuts within a budget chunk, so the two counters run side by side
    uint64_t used = 0, in_budget_chunk = 0, units = 0;
    for (size_t q = 0; q < bytes.size(); ++q) {
        if (bytes[q] > budget) {
            v.ok = false;
            return v;
        }
        const bool over = q > 0 && bytes[q] > budget - used;
        if (q == 0 || over || (cap && in_budget_chunk % cap == 0)) {
            v.first.push_back(q);
            units = 0;
        }
        if (over || q == 0) used = 0, in_budget_chunk = 0;
        v.chunk_of.push_back(v.first.size() - 1);
        v.base.push_back(units);
        used += bytes[q];
        in_budget_chunk += 1;
        units += bytes[q] / unit;
        v.total_units += bytes[q] / unit;
        v.most_units = std::max(v.most_units, units);
        v.most_entries = std::max<uint64_t>(v.most_entries, q + 1 - v.first.back());
    }
    return v;
}

void check_layout(const std::vector<uint64_t>& bytes, uint64_t budget, uint64_t unit, uint64_t cap) {
    const Naive want = naive_layout(bytes, budget, unit, cap);
    ChunkLayout lay;
    const bool ok = itemplan::chunk_layout(bytes.empty() ? nullptr : bytes.data(), bytes.size(), budget, unit, cap, &lay);
    REQUIRE(ok == want.ok);
    if (!ok) return;
    const uint64_t n = bytes.size();
    REQUIRE(lay.cuts.size() == want.first.size() + 1 && lay.chunks() == want.first.size());
    REQUIRE(lay.cuts.front() == 0 && lay.cuts.back() == n);
    REQUIRE(lay.base.size() == n && lay.counts.size() == lay.chunks());
    std::vector<int> covered(n, 0);
    for (uint64_t c = 0; c < lay.chunks(); ++c) {
        REQUIRE(lay.cuts[c] == want.first[c] && lay.cuts[c] < lay.cuts[c + 1]);
        REQUIRE(lay.counts[c] == lay.cuts[c + 1] - lay.cuts[c]);
        REQUIRE(!cap || lay.counts[c] <= cap);
        REQUIRE(lay.base[lay.cuts[c]] == 0);  // every chunk's bases restart
        uint64_t sum = 0;
        for (uint64_t q = lay.cuts[c]; q < lay.cuts[c + 1]; ++q) {
            covered[q] += 1;
            REQUIRE(lay.base[q] == want.base[q] && want.chunk_of[q] == c);
            REQUIRE(bytes[q] <= budget - sum);  // (no wrap: sum <= budget)
            sum += bytes[q];
        }
    }
    for (int x : covered) REQUIRE(x == 1);
    REQUIRE(lay.chunk_units == want.most_units && lay.chunk_entries == want.most_entries);
    REQUIRE(lay.total_units == want.total_units);
}

struct Batch {
    std::vector<uint8_t> residues;  // with `lead` bytes in front of the first sequence
    std::vector<uint64_t> offsets;
    std::vector<msv_aln_item> items;
    uint64_t n() const { return offsets.size() - 1; }
};

msv_aln_item item(uint32_t seq, uint32_t a, uint32_t b) {
    msv_aln_item it{};
    it.seq = seq;
    it.i_from = a;
    it.i_to = b;
    return it;
}

Batch make_batch(std::mt19937_64& rng, const std::vector<uint64_t>& lengths, uint64_t lead) {
    Batch b;
    b.offsets.push_back(lead);
    for (uint64_t L : lengths) b.offsets.push_back(b.offsets.back() + L);
    b.residues.resize(b.offsets.back());
    for (auto& x : b.residues) x = static_cast<uint8_t>(rng() % 251);
    return b;
}

msv_status check(const Batch& b, uint64_t* longest) {
    return itemplan::check_items(b.residues.empty() ? nullptr : b.residues.data(), b.offsets.data(), b.n(),
                                 b.items.empty() ? nullptr : b.items.data(), b.items.size(), longest);
}

// The plan of a checked batch against the restatement: every list per item, the packed bytes from where the caller's
// residues have them.
void check_plan(const Batch& b, uint64_t budget) {
    uint64_t longest = 99;
    REQUIRE(check(b, &longest) == MSV_OK);
    uint64_t want_longest = 0;
    for (uint64_t s = 0; s < b.n(); ++s) want_longest = std::max(want_longest, b.offsets[s + 1] - b.offsets[s]);
    REQUIRE(longest == want_longest);
    const uint64_t m = b.items.size();
    std::vector<uint64_t> bytes(m);
    for (uint64_t q = 0; q < m; ++q) bytes[q] = bytes_of(b.items[q].i_to - b.items[q].i_from + 1);
    ItemBatch plan;
    const bool ok = itemplan::plan_items(b.residues.data(), b.offsets.data(), m ? b.items.data() : nullptr, m, budget,
                                         bytes_of, &plan);
    const Naive want = naive_layout(bytes, budget, 4, 0);
    REQUIRE(ok == want.ok);
    if (!ok) {
        REQUIRE(plan.packed.empty());
        return;
    }
    REQUIRE(plan.poff.size() == m + 1 && plan.poff[0] == 0);
    REQUIRE(plan.bytes == bytes && plan.lc.size() == m && plan.sel.size() == m);
    for (uint64_t q = 0; q < m; ++q) {
        const msv_aln_item& it = b.items[q];
        const uint64_t Le = it.i_to - it.i_from + 1;
        REQUIRE(plan.poff[q + 1] - plan.poff[q] == Le && plan.sel[q] == q);
        REQUIRE(plan.lc[q] == b.offsets[it.seq + 1] - b.offsets[it.seq]);  // the whole sequence's, not the envelope's
        const uint8_t* src = b.residues.data() + b.offsets[it.seq] + it.i_from - 1;
        REQUIRE(std::equal(src, src + Le, plan.packed.begin() + static_cast<std::ptrdiff_t>(plan.poff[q])));
        REQUIRE(plan.lay.base[q] == want.base[q]);
    }
    REQUIRE(plan.packed.size() == plan.poff[m]);
    REQUIRE(plan.lay.chunks() == want.first.size() && plan.lay.chunk_units == want.most_units);
    for (uint64_t c = 0; c < plan.lay.chunks(); ++c) REQUIRE(plan.lay.cuts[c] == want.first[c]);
}

void random_cases() {
    std::mt19937_64 rng(17);
    for (int trial = 0; trial < 400; ++trial) {
        // layouts: sizes in units of 4 and of 24 (a decode row), budgets around the sizes, with and without a cap
        const uint64_t n = rng() % 24, unit = trial % 2 ? 24 : 4, cap = trial % 3 ? 0 : 1 + rng() % 5;
        std::vector<uint64_t> bytes(n);
        for (auto& x : bytes) x = unit * (rng() % 60);
        check_layout(bytes, 1 + rng() % (unit * 150), unit, cap);
        // batches: up to 6 sequences of up to 40 residues behind a lead, up to 12 valid items in any order
        std::vector<uint64_t> lengths(rng() % 7);
        for (auto& L : lengths) L = rng() % 41;
        Batch b = make_batch(rng, lengths, rng() % 9);
        for (uint64_t tries = rng() % 13; tries; --tries) {
            if (lengths.empty()) break;
            const uint32_t s = static_cast<uint32_t>(rng() % lengths.size());
            if (lengths[s] == 0) continue;
            const uint32_t a = 1 + static_cast<uint32_t>(rng() % lengths[s]);
            b.items.push_back(item(s, a, a + static_cast<uint32_t>(rng() % (lengths[s] - a + 1))));
        }
        check_plan(b, 1 + rng() % (bytes_of(40) * 3));
    }
}

void named_edges() {
    std::mt19937_64 rng(19);
    uint64_t longest = 0;
    // m == 0 and n == 0
    Batch none = make_batch(rng, {}, 0);
    check_plan(none, 1);
    Batch no_items = make_batch(rng, {5, 0, 7}, 0);
    check_plan(no_items, 1);
    none.items.push_back(item(0, 1, 1));
    REQUIRE(check(none, &longest) == kBad);  // an item and no sequence
    check_layout({}, 1, 4, 0);
    check_layout({}, 1, 4, 3);

    const uint64_t L = 30;
    Batch b = make_batch(rng, {12, L, 9}, 0);
    auto with = [&](msv_aln_item it) {
        Batch c = b;
        c.items = {item(0, 1, 12), it};
        return c;
    };
    check_plan(with(item(1, 7, 7)), 1 << 20);                              // Le == 1
    check_plan(with(item(1, 1, static_cast<uint32_t>(L))), 1 << 20);       // i_to == L exactly
    REQUIRE(check(with(item(1, 1, static_cast<uint32_t>(L) + 1)), &longest) == kBad);
    REQUIRE(check(with(item(1, 0, 5)), &longest) == kBad);                 // i_from == 0
    REQUIRE(check(with(item(1, 6, 5)), &longest) == kBad);                 // i_from > i_to
    REQUIRE(check(with(item(3, 1, 1)), &longest) == kBad);                 // seq == n
    Batch falling = with(item(1, 1, 5));
    std::swap(falling.offsets[1], falling.offsets[2]);
    REQUIRE(check(falling, &longest) == kBad);                             // offsets that decrease
    Batch too_long = make_batch(rng, {}, 0);
    too_long.offsets = {0, 1ull << 31};
    too_long.residues.assign(1, 0);  // (never read: the refusal comes first)
    REQUIRE(check(too_long, &longest) == MSV_ERR_SEQUENCE_TOO_LONG);
    Batch no_residues = make_batch(rng, {3}, 0);
    REQUIRE(itemplan::check_items(nullptr, no_residues.offsets.data(), 1, nullptr, 0, &longest) == kBad);
    REQUIRE(itemplan::check_items(nullptr, nullptr, 1ull << 32, nullptr, 0, &longest) == kBad);
    REQUIRE(itemplan::check_items(nullptr, nullptr, 0, nullptr, 1ull << 32, &longest) == kBad);

    // offsets[0] != 0: the packed bytes come from residues + offsets[seq] + i_from - 1
    Batch led = make_batch(rng, {12, L, 9}, 5);
    led.items = {item(2, 2, 9), item(0, 1, 12), item(1, 30, 30)};
    check_plan(led, 1 << 20);
    // two overlapping items on one sequence, listed out of sequence order
    led.items = {item(1, 10, 25), item(2, 1, 9), item(1, 20, 30), item(0, 3, 3)};
    check_plan(led, 1 << 20);
    check_plan(led, bytes_of(16) + bytes_of(9));

    // a budget equal to the sum of the first two entries: they share a chunk, the third starts the next at base 0
    const std::vector<uint64_t> three = {400, 240, 80};
    ChunkLayout lay;
    REQUIRE(itemplan::chunk_layout(three.data(), 3, 640, 4, 0, &lay));
    REQUIRE((lay.cuts == std::vector<uint64_t>{0, 2, 3}) && lay.base[1] == 100 && lay.base[2] == 0);
    REQUIRE(lay.chunk_units == 160 && lay.chunk_entries == 2 && lay.total_units == 180);
    check_layout(three, 640, 4, 0);
    // one byte less: the second starts a chunk and the third joins it
    REQUIRE(itemplan::chunk_layout(three.data(), 3, 639, 4, 0, &lay));
    REQUIRE((lay.cuts == std::vector<uint64_t>{0, 1, 3}) && lay.base[1] == 0 && lay.base[2] == 60);
    check_layout(three, 639, 4, 0);
    // a budget one byte under the largest entry
    REQUIRE(!itemplan::chunk_layout(three.data(), 3, 399, 4, 0, &lay));
    REQUIRE(itemplan::chunk_layout(three.data(), 3, 400, 4, 0, &lay) && lay.chunks() == 2);
    // no workspace given is the default one
    REQUIRE(itemplan::chunk_layout(three.data(), 3, 0, 4, 0, &lay) && lay.chunks() == 1);
    const std::vector<uint64_t> huge = {itemplan::kDefaultWorkspace + 4};
    REQUIRE(!itemplan::chunk_layout(huge.data(), 1, 0, 4, 0, &lay));
    // sizes 2^63, 2^63 under a budget of 2^64 - 1: no wrap
    const std::vector<uint64_t> big = {1ull << 63, 1ull << 63};
    REQUIRE(itemplan::chunk_layout(big.data(), 2, ~0ull, 4, 0, &lay));
    REQUIRE(lay.chunks() == 2 && lay.base[1] == 0 && lay.chunk_units == 1ull << 61);
    REQUIRE(!itemplan::chunk_layout(big.data(), 2, (1ull << 63) - 1, 4, 0, &lay));
    // the entry cap with m = 7, n = 3: no chunk over 3 entries, every entry once, bases restart per chunk
    const std::vector<uint64_t> seven(7, 48);
    REQUIRE(itemplan::chunk_layout(seven.data(), 7, 1 << 20, 24, 3, &lay));
    REQUIRE((lay.cuts == std::vector<uint64_t>{0, 3, 6, 7}) && (lay.counts == std::vector<uint32_t>{3, 3, 1}));
    REQUIRE((lay.base == std::vector<uint64_t>{0, 2, 4, 0, 2, 4, 0}) && lay.chunk_units == 6 && lay.chunk_entries == 3);
    check_layout(seven, 1 << 20, 24, 3);
    check_layout(seven, 48 * 5, 24, 3);  // budget chunks of five, each cut again: 3 + 2, 2
    REQUIRE(itemplan::chunk_layout(seven.data(), 7, 48 * 5, 24, 3, &lay));
    REQUIRE((lay.cuts == std::vector<uint64_t>{0, 3, 5, 7}));
}

}  // namespace

int main() {
    random_cases();
    named_edges();
    std::printf("sanitize_item_plan passed\n");
    return 0;
}
