// item_plan.h -- host-only arithmetic the chunked host calls share (the Viterbi trace, decode, align and sample;
// DESIGN 4.8, 4.10, 4.11, 4.14): the extent of a CSR, the layout of a list's entries in workspace-sized chunks, and
// the batch that align and sample make of their envelope items.  No HIP here, so the sanitizer builds run it
// (tests/cpp/sanitize_item_plan.cpp); the device layers launch what it says.
#pragma once

#include <algorithm>
#include <cstdint>
#include <functional>
#include <vector>

#include "msv.h"
#include "vit_trace_plan.h"

namespace itemplan {

// The workspace of a chunked host call that is given none.
using vittrace::kDefaultWorkspace;

// Validates a CSR (offsets non-decreasing) and finds its longest sequence and its residue count.
inline msv_status csr_extent(const uint64_t* offsets, uint64_t n, uint64_t* maxL, uint64_t* total) {
    uint64_t longest = 0;
    for (uint64_t s = 0; s < n; ++s) {
        if (offsets[s + 1] < offsets[s]) return MSV_ERR_INVALID_ARGUMENT;
        longest = std::max<uint64_t>(longest, offsets[s + 1] - offsets[s]);
    }
    *maxL = longest;
    *total = n ? offsets[n] - offsets[0] : 0;
    return MSV_OK;
}

// A list's entries in chunks, each chunk's entries back to back from 0 in units of `unit` bytes.
struct ChunkLayout {
    std::vector<uint64_t> cuts;    // chunk c = entries cuts[c] .. cuts[c + 1] (no entries: {0})
    std::vector<uint64_t> base;    // per entry: where it starts within its chunk, in units
    std::vector<uint32_t> counts;  // per chunk: its entries
    uint64_t chunk_units = 0;      // the largest chunk, in units
    uint64_t chunk_entries = 0;    // the largest chunk, in entries
    uint64_t total_units = 0;      // every chunk's units, summed
    uint64_t chunks() const { return cuts.size() - 1; }
};
// vittrace::chunk_cuts of bytes[0 .. n) under `budget` (0, a call's "no workspace given": kDefaultWorkspace; false, as
// there, when one entry alone exceeds it), each chunk then cut again into runs of at most max_entries entries (0: no
// cap), and the layout of the result.
bool chunk_layout(const uint64_t* bytes, uint64_t n, uint64_t budget, uint64_t unit, uint64_t max_entries,
                  ChunkLayout* out);

// The checks align and sample make of a host CSR and the items on it, in their order: the counts below 2^32, the CSR
// (csr_extent; residues where it has any), its longest sequence below 2^31, every item 1 <= i_from <= i_to <= L on a
// sequence of the batch.
msv_status check_items(const uint8_t* residues, const uint64_t* offsets, uint64_t n, const msv_aln_item* items,
                       uint64_t m, uint64_t* longest);

// Checked items as a batch of their own: item q is sequence q of the CSR (packed, poff).
struct ItemBatch {
    std::vector<uint64_t> poff;   // [m + 1] offsets of the envelopes' residues in `packed`
    std::vector<uint64_t> bytes;  // per item: bytes_of(Le)
    std::vector<uint32_t> lc;     // per item: the length of its whole sequence (the configured length)
    std::vector<uint32_t> sel;    // 0 .. m - 1
    std::vector<uint8_t> packed;
    ChunkLayout lay;              // in 4-byte words
};
// False when one item alone exceeds the budget (nothing is packed then).
bool plan_items(const uint8_t* residues, const uint64_t* offsets, const msv_aln_item* items, uint64_t m,
                uint64_t budget, const std::function<uint64_t(uint64_t Le)>& bytes_of, ItemBatch* out);

}  // namespace itemplan
