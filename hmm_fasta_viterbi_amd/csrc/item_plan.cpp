// item_plan.cpp -- the chunk layout and the item batch of item_plan.h.  No HIP in this translation unit.
#include "item_plan.h"

namespace itemplan {

bool chunk_layout(const uint64_t* bytes, uint64_t n, uint64_t budget, uint64_t unit, uint64_t max_entries,
                  ChunkLayout* out) {
    *out = ChunkLayout{};
    if (!vittrace::chunk_cuts(bytes, n, budget ? budget : kDefaultWorkspace, &out->cuts)) return false;
    if (max_entries) {
        // a launch's list may be capped (seq_queue.h: no longer than the batch): cut again
        std::vector<uint64_t> fine{0};
        for (size_t c = 0; c + 1 < out->cuts.size(); ++c)
            for (uint64_t lo = out->cuts[c]; lo < out->cuts[c + 1]; lo += max_entries)
                fine.push_back(std::min(lo + max_entries, out->cuts[c + 1]));
        out->cuts = fine;
    }
    out->base.resize(n);
    out->counts.resize(out->chunks());
    for (uint64_t c = 0; c < out->chunks(); ++c) {
        uint64_t at = 0;
        for (uint64_t q = out->cuts[c]; q < out->cuts[c + 1]; ++q) {
            out->base[q] = at;
            at += bytes[q] / unit;
        }
        out->counts[c] = static_cast<uint32_t>(out->cuts[c + 1] - out->cuts[c]);
        out->chunk_units = std::max(out->chunk_units, at);
        out->chunk_entries = std::max<uint64_t>(out->chunk_entries, out->counts[c]);
        out->total_units += at;
    }
    return true;
}

msv_status check_items(const uint8_t* residues, const uint64_t* offsets, uint64_t n, const msv_aln_item* items,
                       uint64_t m, uint64_t* longest) {
    if (n >= (1ull << 32) || m >= (1ull << 32)) return MSV_ERR_INVALID_ARGUMENT;
    uint64_t total = 0;
    *longest = 0;
    const msv_status s = n ? csr_extent(offsets, n, longest, &total) : MSV_OK;
    if (s != MSV_OK) return s;
    if (total && !residues) return MSV_ERR_INVALID_ARGUMENT;
    if (*longest >= (1ull << 31)) return MSV_ERR_SEQUENCE_TOO_LONG;
    for (uint64_t q = 0; q < m; ++q) {
        const msv_aln_item& it = items[q];
        if (it.seq >= n || it.i_from < 1 || it.i_from > it.i_to || it.i_to > offsets[it.seq + 1] - offsets[it.seq])
            return MSV_ERR_INVALID_ARGUMENT;
    }
    return MSV_OK;
}

bool plan_items(const uint8_t* residues, const uint64_t* offsets, const msv_aln_item* items, uint64_t m,
                uint64_t budget, const std::function<uint64_t(uint64_t Le)>& bytes_of, ItemBatch* out) {
    *out = ItemBatch{};
    out->poff.assign(m + 1, 0);
    out->bytes.resize(m);
    out->lc.resize(m);
    out->sel.resize(m);
    for (uint64_t q = 0; q < m; ++q) {
        const uint64_t Le = items[q].i_to - items[q].i_from + 1;
        out->poff[q + 1] = out->poff[q] + Le;
        out->bytes[q] = bytes_of(Le);
        out->lc[q] = static_cast<uint32_t>(offsets[items[q].seq + 1] - offsets[items[q].seq]);
        out->sel[q] = static_cast<uint32_t>(q);
    }
    if (!chunk_layout(out->bytes.data(), m, budget, sizeof(uint32_t), 0, &out->lay)) return false;
    out->packed.resize(out->poff[m]);
    for (uint64_t q = 0; q < m; ++q)
        std::copy_n(residues + offsets[items[q].seq] + items[q].i_from - 1, out->poff[q + 1] - out->poff[q],
                    out->packed.begin() + static_cast<std::ptrdiff_t>(out->poff[q]));
    return true;
}

}  // namespace itemplan
