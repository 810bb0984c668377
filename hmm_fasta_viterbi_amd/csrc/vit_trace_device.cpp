// vit_trace_device.cpp -- C-ABI of the Viterbi trace (msv.h "Viterbi traces") on the HIP runtime.
//
// msv_vit_trace_batch stages the batch like the other host calls (the profile's CsrStaging, a StreamDrain on
// early returns), lays the select list out in chunks whose back-pointers fit the workspace (item_plan.h's
// chunk_layout over vit_trace_plan.cpp's cuts), and per chunk runs the fill kernel on a launch slot of the profile,
// the walk's counting pass, an exclusive scan of the counts on the host (the output is sized exactly from it), and
// the walk's writing pass.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <new>
#include <vector>

#include "hip_rt.h"
#include "host_cpu.h"
#include "msv.h"
#include "vit_profile.h"
#include "vit_trace.h"
#include "vit_trace_plan.h"

using msvrt::DeviceGuard;
using msvrt::hip_status;

struct msv_vit_traces {
    std::vector<float> scores;
    std::vector<uint64_t> dom_off;  // count + 1
    std::vector<msv_vit_domain> domains;
    std::vector<uint8_t> ops;
    msv_vit_trace_stats stats{};
};

namespace {

// The profile's trace plan, its tables and its grid, made on the first use.
msv_status ensure_plan(msv_vit_profile* p) {
    vitdev::TraceState& t = p->trace;
    if (t.plan >= 0) return MSV_OK;
    const int plan = vittrace::pick_plan(p->model_length - 1);
    if (plan < 0) return MSV_ERR_UNSUPPORTED_MODEL;
    const vittrace::Plan& pl = vittrace::kPlans[plan];
    const msv_host::VitTables tab = msv_host::vit_tables(p->msc.data(), p->isc_tab.data(), p->tsc.data(),
                                                         p->model_length, pl.S, pl.team, p->isc);
    MSV_HIP(stagedev::upload_pairs(t.d_etab, tab.et));
    MSV_HIP(stagedev::upload_pairs(t.d_ttab, tab.tt));
    if (p->isc) MSV_HIP(stagedev::upload_pairs(t.d_itab, tab.it));
    int blocks = 0;
    MSV_HIP(msvrt::resident_blocks(p->device, vittrace::fill_kernel(plan), static_cast<int>(pl.lanes()), &blocks));
    MSV_HIP(t.t0.create(hipEventDefault));
    MSV_HIP(t.t1.create(hipEventDefault));
    MSV_HIP(t.t2.create(hipEventDefault));
    MSV_HIP(t.t3.create(hipEventDefault));
    t.blocks = static_cast<uint32_t>(std::max(1, blocks));
    t.plan = plan;
    return MSV_OK;
}

// The host lists a chunk's copies read or write: owned by the call, so that they outlive the stream's drain on
// an early return.
struct ChunkLists {
    std::vector<uint64_t> dom_off, ops_off;
    std::vector<uint32_t> counts;
};

// One chunk: the select entries sel[0 .. m), each from word base[j] of the chunk's `words`, appended to `out` at
// entry `first`.
msv_status run_chunk(msv_vit_profile* p, const uint32_t* sel, const uint64_t* base, uint64_t words, uint64_t m,
                     uint64_t first, hipStream_t st, ChunkLists& h, msv_vit_traces* out) {
    vitdev::TraceState& t = p->trace;
    const vittrace::Plan& pl = vittrace::kPlans[t.plan];
    msvrt::CsrStaging& sg = p->staged;
    MSV_HIP(t.d_select.reserve(m));
    MSV_HIP(t.d_base.reserve(m));
    MSV_HIP(t.d_counts.reserve(2 * m));
    MSV_HIP(t.d_scores.reserve(m));
    MSV_HIP(t.d_dom_off.reserve(m + 1));
    MSV_HIP(t.d_ops_off.reserve(m + 1));
    MSV_HIP(hipMemcpyAsync(t.d_select, sel, m * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    MSV_HIP(hipMemcpyAsync(t.d_base, base, m * sizeof(uint64_t), hipMemcpyHostToDevice, st));

    vittrace::FillArgs f{};
    f.etab = t.d_etab;
    f.itab = p->isc ? t.d_itab.get() : nullptr;
    f.ttab = t.d_ttab;
    f.residues = sg.d_res;
    f.offsets = sg.d_off;
    f.select = t.d_select;
    f.base = t.d_base;
    f.lentab = p->d_lentab;
    f.ws = t.d_ws;
    f.scores = t.d_scores;
    f.errors = p->d_words + stagedev::kHostErrWord;
    f.n_items = static_cast<uint32_t>(m);
    f.lentab_n = p->lentab_n;
    f.tr_B_Mk = p->tr_B_Mk;
    f.tr_E_C = p->tr_E_C;
    f.tr_E_J = p->tr_E_J;
    const uint32_t blocks = static_cast<uint32_t>(std::min<uint64_t>(t.blocks, m));
    MSV_HIP(hipEventRecord(t.t0, st));
    MSV_HIP(p->kernels.run(st, true, p->d_words.get(), 2, [&](uint32_t* counter) {
        f.counter = counter;
        return vittrace::launch_fill(t.plan, blocks, f, st);
    }));
    MSV_HIP(hipEventRecord(t.t1, st));

    vittrace::WalkArgs w{};
    w.offsets = sg.d_off;
    w.select = t.d_select;
    w.base = t.d_base;
    w.ws = t.d_ws;
    w.scores = t.d_scores;
    w.counts = t.d_counts;
    w.n_items = static_cast<uint32_t>(m);
    w.S = static_cast<uint32_t>(pl.S);
    w.words = pl.words();
    w.lanes = pl.lanes();
    // pass 1: the counts
    MSV_HIP(hipEventRecord(t.t2, st));
    MSV_HIP(vittrace::launch_walk(w, st));
    MSV_HIP(hipEventRecord(t.t3, st));
    std::vector<uint32_t>& counts = h.counts;
    counts.assign(2 * m, 0);
    MSV_HIP(hipMemcpyAsync(counts.data(), t.d_counts, 2 * m * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    MSV_HIP(hipMemcpyAsync(out->scores.data() + first, t.d_scores, m * sizeof(float), hipMemcpyDeviceToHost, st));
    MSV_HIP(hipStreamSynchronize(st));
    out->stats.fill_ms += msvrt::elapsed(t.t0, t.t1);
    out->stats.walk_ms += msvrt::elapsed(t.t2, t.t3);
    out->stats.chunks += 1;
    out->stats.pointer_bytes += words * sizeof(uint32_t);

    // the exclusive scan of the counts: each entry's exact ranges
    std::vector<uint64_t>&dom_off = h.dom_off, &ops_off = h.ops_off;
    dom_off.assign(m + 1, 0);
    ops_off.assign(m + 1, 0);
    for (uint64_t j = 0; j < m; ++j) {
        dom_off[j + 1] = dom_off[j] + counts[2 * j];
        ops_off[j + 1] = ops_off[j] + counts[2 * j + 1];
    }
    const uint64_t nd = dom_off[m], no = ops_off[m];
    const uint64_t d0 = out->domains.size(), o0 = out->ops.size();
    for (uint64_t j = 0; j < m; ++j) out->dom_off[first + j + 1] = d0 + dom_off[j + 1];
    if (nd == 0) return MSV_OK;
    // pass 2: domains and ops at their exact offsets
    MSV_HIP(t.d_domains.reserve(nd));
    MSV_HIP(t.d_ops.reserve(no));
    MSV_HIP(hipMemcpyAsync(t.d_dom_off, dom_off.data(), (m + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    MSV_HIP(hipMemcpyAsync(t.d_ops_off, ops_off.data(), (m + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    w.dom_off = t.d_dom_off;
    w.ops_off = t.d_ops_off;
    w.domains = t.d_domains;
    w.ops = t.d_ops;
    MSV_HIP(hipEventRecord(t.t2, st));
    MSV_HIP(vittrace::launch_walk(w, st));
    MSV_HIP(hipEventRecord(t.t3, st));
    out->domains.resize(d0 + nd);
    out->ops.resize(o0 + no);
    MSV_HIP(hipMemcpyAsync(out->domains.data() + d0, t.d_domains, nd * sizeof(msv_vit_domain), hipMemcpyDeviceToHost,
                           st));
    MSV_HIP(hipMemcpyAsync(out->ops.data() + o0, t.d_ops, no, hipMemcpyDeviceToHost, st));
    MSV_HIP(hipStreamSynchronize(st));
    out->stats.walk_ms += msvrt::elapsed(t.t2, t.t3);
    for (uint64_t d = d0; d < d0 + nd; ++d) out->domains[d].ops_begin += o0;
    return MSV_OK;
}

}  // namespace

extern "C" {

msv_status msv_vit_trace_batch(msv_vit_profile* p, const uint8_t* residues, const uint64_t* offsets, uint64_t n,
                               const uint32_t* select, uint64_t n_select, uint64_t workspace_bytes,
                               msv_vit_traces** traces) {
    if (!p || !traces || (n && !offsets)) return MSV_ERR_INVALID_ARGUMENT;
    *traces = nullptr;
    if (n >= (1ull << 32) || (select && n_select >= (1ull << 32))) return MSV_ERR_INVALID_ARGUMENT;
    uint64_t longest = 0, total = 0;
    msv_status s = n ? msvrt::csr_extent(offsets, n, &longest, &total) : MSV_OK;
    if (s != MSV_OK) return s;
    if (total && !residues) return MSV_ERR_INVALID_ARGUMENT;
    std::vector<uint32_t> sel;
    if (select) {
        sel.assign(select, select + n_select);
        for (uint32_t x : sel)
            if (x >= n) return MSV_ERR_INVALID_ARGUMENT;
    } else {
        sel.resize(n);
        for (uint64_t q = 0; q < n; ++q) sel[q] = static_cast<uint32_t>(q);
    }
    const uint64_t ns = sel.size();
    auto* out = new (std::nothrow) msv_vit_traces;
    if (!out) return MSV_ERR_OUT_OF_MEMORY;
    out->scores.assign(ns, 0.0f);
    out->dom_off.assign(ns + 1, 0);
    if (ns == 0) {
        *traces = out;
        return MSV_OK;
    }
    auto fail = [&](msv_status st) {
        delete out;
        return st;
    };
    DeviceGuard g(p->device);
    if (!g.ok) return fail(MSV_ERR_NO_DEVICE);
    if ((s = ensure_plan(p)) != MSV_OK) return fail(s);
    // (a sequence too long for any length table is the scoring calls' refusal, ahead of the workspace's)
    if ((s = msv_vit_profile_reserve_length(p, longest)) != MSV_OK) return fail(s);
    const vittrace::Plan& pl = vittrace::kPlans[p->trace.plan];
    // the chunk cuts, before anything is launched: a sequence that alone exceeds the workspace is refused here
    std::vector<uint64_t> bytes(ns);
    for (uint64_t q = 0; q < ns; ++q)
        bytes[q] = vittrace::sequence_words(pl, offsets[sel[q] + 1] - offsets[sel[q]]) * sizeof(uint32_t);
    itemplan::ChunkLayout lay;  // in words
    if (!itemplan::chunk_layout(bytes.data(), ns, workspace_bytes, sizeof(uint32_t), 0, &lay))
        return fail(MSV_ERR_OUT_OF_MEMORY);
    const std::vector<uint64_t>& cuts = lay.cuts;
    hipError_t e = p->trace.d_ws.reserve(lay.chunk_units);
    if (e != hipSuccess) return fail(hip_status(e));
    hipStream_t st = p->stream;
    ChunkLists lists;
    {
        // an early error return leaves no copy queued that reads the pinned offsets or the chunk's host lists
        msvrt::StreamDrain drain(st);
        e = p->staged.upload(residues, offsets, 0, n, true, st, st);
        s = hip_status(e);
        for (size_t c = 0; s == MSV_OK && c + 1 < cuts.size(); ++c) {
            const uint64_t last = cuts[c + 1] - 1, words = lay.base[last] + bytes[last] / sizeof(uint32_t);
            s = run_chunk(p, sel.data() + cuts[c], lay.base.data() + cuts[c], words, cuts[c + 1] - cuts[c], cuts[c],
                          st, lists, out);
        }
    }  // (drained: every chunk has synchronised, or an error has)
    p->trace.d_ws.reset();  // the workspace is not kept between calls
    if (s != MSV_OK) return fail(s);
    s = stagedev::read_errors(p, stagedev::kHostErrWord, st);
    if (s != MSV_OK && s != MSV_ERR_BAD_RESIDUE && s != MSV_ERR_SEQUENCE_TOO_LONG) return fail(s);
    *traces = out;
    return s;
}

uint64_t msv_vit_traces_count(const msv_vit_traces* t) { return t ? t->scores.size() : 0; }
uint64_t msv_vit_traces_domains(const msv_vit_traces* t) { return t ? t->domains.size() : 0; }
uint64_t msv_vit_traces_ops(const msv_vit_traces* t) { return t ? t->ops.size() : 0; }

msv_status msv_vit_traces_copy(const msv_vit_traces* t, float* scores, uint64_t* domain_offsets,
                               msv_vit_domain* domains, uint8_t* ops) {
    if (!t) return MSV_ERR_INVALID_ARGUMENT;
    if (scores) std::copy(t->scores.begin(), t->scores.end(), scores);
    if (domain_offsets) std::copy(t->dom_off.begin(), t->dom_off.end(), domain_offsets);
    if (domains) std::copy(t->domains.begin(), t->domains.end(), domains);
    if (ops) std::copy(t->ops.begin(), t->ops.end(), ops);
    return MSV_OK;
}

void msv_vit_traces_free(msv_vit_traces* t) { delete t; }

msv_status msv_vit_traces_stats(const msv_vit_traces* t, msv_vit_trace_stats* out) {
    if (!t || !out) return MSV_ERR_INVALID_ARGUMENT;
    *out = t->stats;
    return MSV_OK;
}

msv_status msv_vit_trace_describe(msv_vit_profile* p, msv_vit_trace_info* out) {
    if (!p || !out) return MSV_ERR_INVALID_ARGUMENT;
    DeviceGuard g(p->device);
    if (!g.ok) return MSV_ERR_NO_DEVICE;
    const msv_status s = ensure_plan(p);
    if (s != MSV_OK) return s;
    const vittrace::Plan& pl = vittrace::kPlans[p->trace.plan];
    std::memset(out, 0, sizeof(*out));
    std::snprintf(out->plan, sizeof(out->plan), "%s", pl.name);
    out->states_per_lane = static_cast<uint32_t>(pl.S);
    out->lanes_per_sequence = pl.lanes();
    out->capacity = pl.capacity();
    out->words_per_lane = pl.words();
    out->blocks = p->trace.blocks;
    out->default_workspace_bytes = vittrace::kDefaultWorkspace;
    msvrt::kernel_footprint(vittrace::fill_kernel(p->trace.plan), &out->scratch_bytes, &out->lds_bytes);
    return MSV_OK;
}

}  // extern "C"
