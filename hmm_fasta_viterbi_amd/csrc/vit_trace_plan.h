// vit_trace_plan.h -- host-only arithmetic of the Viterbi trace (msv.h): the compiled plans, the
// back-pointer layout of a plan and the cuts of a select list into workspace-sized chunks.  No HIP here, so the
// sanitizer builds run it (tests/cpp/sanitize_trace.cpp); vit_trace.hip, the device layer and the tests share
// this one definition.
#pragma once

#include <cstdint>
#include <vector>

namespace vittrace {

constexpr int kCellBits = 4;       // M source 2 bits, I source 1, D source 1
constexpr int kCellsPerWord = 8;   // cells of one uint32
constexpr uint64_t kDefaultWorkspace = 1ull << 30;

// cell bits
constexpr uint32_t kFromM = 0, kFromI = 1, kFromD = 2, kFromB = 3;  // M's source (bits 0-1)
constexpr uint32_t kIFromI = 4;                                     // I's source (bit 2): 0 M, 1 I
constexpr uint32_t kDFromD = 8;                                     // D's source (bit 3): 0 M, 1 D
// row record: E's argmax k in the low 16 bits, then the flags
constexpr uint32_t kRecKMask = 0xffffu;
constexpr uint32_t kRecCFromE = 1u << 16, kRecJFromE = 1u << 17, kRecBFromJ = 1u << 18;

// One compiled fill kernel: a workgroup of `team` waves per sequence, lane v = wave * 64 + lane holds the S
// consecutive states v * S + 1 .. v * S + S (vit_tables' team layout).
struct Plan {
    const char* name;
    int S;
    int team;
    constexpr uint32_t lanes() const { return 64u * static_cast<uint32_t>(team); }
    constexpr uint32_t words() const { return static_cast<uint32_t>((S + kCellsPerWord - 1) / kCellsPerWord); }
    constexpr uint32_t capacity() const { return lanes() * static_cast<uint32_t>(S); }
};
// by rising capacity; vit_trace.hip instantiates one kernel per entry, in this order
constexpr Plan kPlans[] = {
    {"vit_trace_s8_w1", 8, 1},
    {"vit_trace_s8_w4", 8, 4},
    {"vit_trace_s16_w4", 16, 4},
};
constexpr int kPlanCount = static_cast<int>(sizeof(kPlans) / sizeof(kPlans[0]));

// The first plan that holds `states` (LENG), or -1.
int pick_plan(uint32_t states);

struct Cell {
    uint32_t word, lane, shift;
};
// Where node k (1 .. capacity) keeps its 4 bits within a row of words() x lanes() uint32.
constexpr Cell cell_of(const Plan& p, uint32_t k) {
    const uint32_t v = (k - 1) / static_cast<uint32_t>(p.S), q = (k - 1) % static_cast<uint32_t>(p.S);
    return Cell{q / kCellsPerWord, v, (q % kCellsPerWord) * kCellBits};
}
// uint32 words of one sequence's workspace: L rows of back-pointers, then L row records.
constexpr uint64_t sequence_words(const Plan& p, uint64_t L) {
    return L * (static_cast<uint64_t>(p.words()) * p.lanes() + 1);
}

// Greedy cuts of `bytes` (one entry per selected sequence, in the caller's order) into chunks whose sum is at
// most `workspace`: returns false when one sequence alone exceeds it, else cuts = {0, ..., n} (n = 0: {0}).
bool chunk_cuts(const uint64_t* bytes, uint64_t n, uint64_t workspace, std::vector<uint64_t>* cuts);

}  // namespace vittrace
