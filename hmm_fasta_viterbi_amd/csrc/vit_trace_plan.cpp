// vit_trace_plan.cpp -- host-only half of the Viterbi trace (vit_trace_plan.h): plan choice, the back-pointer
// layout and the chunk cuts, and their C entry points of msv.h.  No HIP in this translation unit.
#include "vit_trace_plan.h"

#include "msv.h"

namespace vittrace {

int pick_plan(uint32_t states) {
    for (int i = 0; i < kPlanCount; ++i)
        if (states <= kPlans[i].capacity()) return i;
    return -1;
}

bool chunk_cuts(const uint64_t* bytes, uint64_t n, uint64_t workspace, std::vector<uint64_t>* cuts) {
    cuts->assign(1, 0);
    uint64_t used = 0;
    for (uint64_t q = 0; q < n; ++q) {
        if (bytes[q] > workspace) return false;
        if (bytes[q] > workspace - used) {  // (no overflow: used <= workspace)
            cuts->push_back(q);
            used = 0;
        }
        used += bytes[q];
    }
    if (n) cuts->push_back(n);
    return true;
}

}  // namespace vittrace

extern "C" {

int msv_vit_trace_plan_count(void) { return vittrace::kPlanCount; }

const char* msv_vit_trace_plan_name(int i) {
    return (i >= 0 && i < vittrace::kPlanCount) ? vittrace::kPlans[i].name : "";
}

uint32_t msv_vit_trace_plan_capacity(int i) {
    return (i >= 0 && i < vittrace::kPlanCount) ? vittrace::kPlans[i].capacity() : 0;
}

msv_status msv_vit_trace_plan_cell(int i, uint32_t k, uint32_t* word, uint32_t* lane, uint32_t* shift, uint32_t* words,
                                   uint32_t* lanes) {
    if (i < 0 || i >= vittrace::kPlanCount) return MSV_ERR_INVALID_ARGUMENT;
    const vittrace::Plan& p = vittrace::kPlans[i];
    if (k < 1 || k > p.capacity()) return MSV_ERR_INVALID_ARGUMENT;
    const vittrace::Cell c = vittrace::cell_of(p, k);
    if (word) *word = c.word;
    if (lane) *lane = c.lane;
    if (shift) *shift = c.shift;
    if (words) *words = p.words();
    if (lanes) *lanes = p.lanes();
    return MSV_OK;
}

uint64_t msv_vit_trace_sequence_bytes(int i, uint64_t L) {
    if (i < 0 || i >= vittrace::kPlanCount) return 0;
    return vittrace::sequence_words(vittrace::kPlans[i], L) * sizeof(uint32_t);
}

msv_status msv_vit_trace_chunk_cuts(const uint64_t* bytes, uint64_t n, uint64_t workspace_bytes, uint64_t* cuts,
                                    uint64_t* n_chunks) {
    if (!n_chunks || (n && !bytes)) return MSV_ERR_INVALID_ARGUMENT;
    std::vector<uint64_t> c;
    if (!vittrace::chunk_cuts(bytes, n, workspace_bytes, &c)) return MSV_ERR_OUT_OF_MEMORY;
    *n_chunks = c.size() - 1;
    if (cuts)
        for (size_t j = 0; j < c.size(); ++j) cuts[j] = c[j];
    return MSV_OK;
}

}  // extern "C"
