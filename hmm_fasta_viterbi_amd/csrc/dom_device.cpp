// dom_device.cpp -- C-ABI of the domain stage (msv.h) on the HIP runtime.
//
// A msv_dom_profile is a stage profile (stage_profile.h) of one compiled variant of dom_kernel.hip: Forward's odds
// tables and scan constants for the recording kernel, the own-node transition arrays and the mirrored scan constants
// for the Backward kernel.  A decode is two persistent launches per chunk of selected sequences (each on its own
// launch slot), the chunks laid out in record rows by item_plan.h's chunk_layout; the envelope rule follows on the
// device.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <new>
#include <vector>

#include "dom_host.h"
#include "dom_kernel.h"
#include "dom_profile.h"
#include "hip_rt.h"
#include "host_cpu.h"
#include "msv.h"
#include "msv_kernel.h"
#include "stage_profile.h"

using msvrt::csr_extent;
using msvrt::DeviceBuffer;
using msvrt::DeviceGuard;
using msvrt::hip_status;
using stagedev::kErrWord;
using stagedev::kHostErrWord;

struct msv_dom_result {
    std::vector<float> fwd, bck, begin, end, occ;
    std::vector<uint64_t> res_off, reg_off;
    std::vector<msv_dom_region> regions;
    msv_dom_stats stats{};
};

namespace {

using msvrt::elapsed;
using msvrt::fill_nan;

float odds(float log_score) { return static_cast<float>(std::exp(static_cast<double>(log_score))); }

// Lays the variant's tables out (msv_host::dom_tables) and uploads them, all or none.
msv_status install(msv_dom_profile* p, const domk::DomVariant* v) {
    const msv_host::DomTables t =
        msv_host::dom_tables(p->msc.data(), p->isc_tab.data(), p->tsc.data(), p->model_length, v->S, p->isc);
    DeviceBuffer<float2> de, di, dt, db;
    DeviceBuffer<float> ds, dbs;
    hipError_t e;
    if ((e = stagedev::upload_pairs(de, t.fwd.et)) != hipSuccess ||
        (e = stagedev::upload_pairs(dt, t.fwd.tt)) != hipSuccess ||
        (e = stagedev::upload_pairs(db, t.bt)) != hipSuccess ||
        (e = ds.replace_with(t.fwd.scan.data(), t.fwd.scan.size())) != hipSuccess ||
        (e = dbs.replace_with(t.bscan.data(), t.bscan.size())) != hipSuccess ||
        (p->isc && (e = stagedev::upload_pairs(di, t.fwd.it)) != hipSuccess))
        return hip_status(e);
    int bck_blocks = 0;
    MSV_HIP(msvrt::resident_blocks(p->device, v->bck_fn, v->waves * 64, &bck_blocks));
    const msv_status s = stagedev::adopt_tables(p, v->fn, v->waves * 64, de, di, dt);  // synchronises the device
    if (s != MSV_OK) return s;
    p->d_scan = std::move(ds);
    p->d_btab = std::move(db);
    p->d_bscan = std::move(dbs);
    p->bck_blocks = static_cast<uint32_t>(std::max(1, bck_blocks));
    p->v = v;
    return MSV_OK;
}

// What one decode launch works on beyond the batch
struct Outputs {
    float* fwd = nullptr;
    float* bck = nullptr;
    float* begin = nullptr;
    float* end = nullptr;
    float* occ = nullptr;
    uint32_t* records = nullptr;
    const uint64_t* item_rows = nullptr;
};

domk::DomArgs batch_args(msv_dom_profile* p, const uint8_t* d_residues, const uint64_t* d_offsets, uint64_t n,
                         const uint32_t* d_select, const uint32_t* d_select_count, uint32_t* errors) {
    domk::DomArgs a{};
    a.etab = p->d_etab;
    a.itab = p->d_itab ? p->d_itab.get() : p->d_etab.get();
    a.residues = d_residues;
    a.offsets = d_offsets;
    a.select = d_select;
    a.select_count = d_select ? d_select_count : nullptr;
    a.lentab = p->d_lentab;
    a.errors = errors;
    a.n = n;
    a.lentab_n = p->lentab_n;
    a.tBM = p->tBM;
    a.tEC = p->tEC;
    a.tEJ = p->tEJ;
    return a;
}

// One persistent launch on the next launch slot, over at most `items` list entries, with the grid of the kernel at
// hand.
msv_status run_kernel(msv_dom_profile* p, const void* fn, uint32_t grid, hipStream_t st, uint64_t items,
                      domk::DomArgs& a) {
    return stagedev::run(p, st, items, static_cast<uint64_t>(p->v->waves), grid,
                         [&](uint32_t blocks, uint32_t* counter) {
                             a.counter = counter;
                             return domk::dom_launch(fn, p->v->waves, blocks, a, st);
                         });
}

// The recording launch (records null: the Forward score alone).
msv_status launch_forward(msv_dom_profile* p, domk::DomArgs a, const Outputs& o, uint64_t items, hipStream_t st) {
    a.ttab = p->d_ttab;
    a.scan = p->d_scan;
    a.scores = o.fwd;
    a.records = o.records;
    a.item_rows = o.item_rows;
    return run_kernel(p, p->v->fn, p->blocks, st, items, a);
}

msv_status launch_backward(msv_dom_profile* p, domk::DomArgs a, const Outputs& o, uint64_t items, hipStream_t st) {
    a.ttab = p->d_btab;
    a.scan = p->d_bscan;
    a.scores = o.bck;
    a.fwd_scores = o.fwd;
    a.records = o.records;
    a.item_rows = o.item_rows;
    a.begin = o.begin;
    a.end = o.end;
    a.occ = o.occ;
    return run_kernel(p, p->v->bck_fn, p->bck_blocks, st, items, a);
}

// stage_profile.h's launch shape: the recording kernel's Forward score, nothing recorded
msv_status launch(msv_dom_profile* p, const uint8_t* d_residues, const uint64_t* d_offsets, uint64_t n,
                  const uint32_t* d_select, const uint32_t* d_select_count, float* d_scores, hipStream_t st,
                  uint32_t* errors) {
    Outputs o;
    o.fwd = d_scores;
    return launch_forward(p, batch_args(p, d_residues, d_offsets, n, d_select, d_select_count, errors), o, n, st);
}

}  // namespace

extern "C" {

void msv_dom_profile_destroy(msv_dom_profile* p) { stagedev::close(p); }

msv_status msv_dom_profile_reserve_length(msv_dom_profile* p, uint64_t max_length) {
    return stagedev::reserve_length(p, max_length, [](uint32_t L, float2& t) {
        float loop, move;
        msv_sequence_transitions(L, &loop, &move);
        t.x = odds(loop);
        t.y = odds(move);
    });
}

msv_status msv_dom_profile_create(int device, const float* match_scores, const float* insert_scores,
                                  const float* transition_scores, uint32_t model_length, float tr_B_Mk, float tr_E_C,
                                  float tr_E_J, msv_dom_profile** out) {
    msv_status s = stagedev::check_model(match_scores, transition_scores, model_length, out);
    if (s != MSV_OK) return s;
    const domk::DomVariant* v = stagedev::pick(domk::dom_variants, model_length - 1, insert_scores != nullptr,
                                               [](const domk::DomVariant&) { return true; });
    if (!v) return MSV_ERR_UNSUPPORTED_MODEL;
    if ((s = stagedev::check_device(device)) != MSV_OK) return s;
    return stagedev::open(device, match_scores, insert_scores, transition_scores, model_length, out,
                          [&](msv_dom_profile* p) {
                              p->tBM = odds(tr_B_Mk);
                              p->tEC = odds(tr_E_C);
                              p->tEJ = odds(tr_E_J);
                              p->tr_B_Mk = tr_B_Mk;
                              p->tr_E_C = tr_E_C;
                              p->tr_E_J = tr_E_J;
                              const msv_status si = install(p, v);
                              return si == MSV_OK
                                         ? msv_dom_profile_reserve_length(p, stagedev::kDefaultMaxLength - 1)
                                         : si;
                          });
}

msv_status msv_dom_profile_create_from_hmm(int device, const msv_hmm* hmm, int insert_mode, msv_dom_profile** out) {
    return stagedev::create_from_hmm(device, hmm, insert_mode, out, msv_dom_profile_create);
}

msv_status msv_dom_profile_describe(const msv_dom_profile* p, msv_dom_info* out) {
    if (!p || !out || out->struct_size < sizeof(uint32_t)) return MSV_ERR_INVALID_ARGUMENT;
    msv_dom_info info;
    std::memset(&info, 0, sizeof(info));
    info.model_length = p->model_length;
    info.states_per_lane = static_cast<uint32_t>(p->v->S);
    info.match_in_lds = p->v->elds ? 1u : 0u;
    info.insert_scores = p->v->isc ? 1u : 0u;
    info.waves_per_block = static_cast<uint32_t>(p->v->waves);
    info.blocks = p->blocks;
    info.backward_blocks = p->bck_blocks;
    info.max_length = p->lentab_n ? p->lentab_n - 1 : 0;
    info.device = p->device;
    std::snprintf(info.variant, sizeof(info.variant), "%s", p->v->name);
    uint32_t bck_scratch = 0;
    msvrt::kernel_footprint(p->v->fn, &info.scratch_bytes, &info.lds_bytes);
    msvrt::kernel_footprint(p->v->bck_fn, &bck_scratch, &info.backward_lds_bytes);
    info.scratch_bytes = std::max(info.scratch_bytes, bck_scratch);
    msv_host::write_sized(out, info);
    return MSV_OK;
}

int msv_dom_variant_count(void) { return stagedev::variant_count(domk::dom_variants); }

const char* msv_dom_variant_name(int i) { return stagedev::variant_name(domk::dom_variants, i); }

msv_status msv_dom_profile_set_variant(msv_dom_profile* p, const char* name) {
    return stagedev::set_variant(p, domk::dom_variants, name, install);
}

msv_status msv_dom_profile_bind_stream(msv_dom_profile* p, void* stream) { return stagedev::bind_stream(p, stream); }

msv_status msv_dom_profile_check(msv_dom_profile* p, void* stream) { return stagedev::check(p, stream); }

msv_status msv_dom_score_batch_device(msv_dom_profile* p, const uint8_t* d_residues, uint64_t residues_len,
                                      const uint64_t* d_offsets, uint64_t n, const uint32_t* d_select,
                                      const uint32_t* d_select_count, float* d_scores, void* stream) {
    return stagedev::score_batch_device(p, d_residues, residues_len, d_offsets, n, d_select, d_select_count, d_scores,
                                        stream, launch);
}

msv_status msv_dom_score_batch(msv_dom_profile* p, const uint8_t* residues, const uint64_t* offsets, uint64_t n,
                               float* scores, void* stream) {
    return stagedev::score_batch_host(p, residues, offsets, n, scores, stream, msv_dom_profile_reserve_length, launch);
}

msv_status msv_dom_decode_batch_device(msv_dom_profile* p, const uint8_t* d_residues, uint64_t residues_len,
                                       const uint64_t* d_offsets, uint64_t n, const uint32_t* d_select,
                                       const uint32_t* d_select_count, float* d_fwd_scores, float* d_bck_scores,
                                       float* d_begin, float* d_end, float* d_occ, void* d_workspace,
                                       uint64_t workspace_bytes, void* stream) {
    if (!p || (n && (!d_offsets || !d_fwd_scores || !d_bck_scores || !d_workspace))) return MSV_ERR_INVALID_ARGUMENT;
    if (n && residues_len && (!d_residues || !d_begin || !d_end || !d_occ)) return MSV_ERR_INVALID_ARGUMENT;
    if (d_select_count && !d_select) return MSV_ERR_INVALID_ARGUMENT;
    if (n == 0) return MSV_OK;
    // sequence s records offsets[s + 1] - offsets[s] + 1 rows from row offsets[s] + s
    if (workspace_bytes / (domk::kRowWords * sizeof(uint32_t)) < residues_len + n) return MSV_ERR_OUT_OF_MEMORY;
    DeviceGuard g(p->device);
    if (!g.ok) return MSV_ERR_NO_DEVICE;
    hipStream_t st = stagedev::stream_of(p, stream);
    Outputs o;
    o.fwd = d_fwd_scores;
    o.bck = d_bck_scores;
    o.begin = d_begin;
    o.end = d_end;
    o.occ = d_occ;
    o.records = static_cast<uint32_t*>(d_workspace);
    const domk::DomArgs a = batch_args(p, d_residues, d_offsets, n, d_select, d_select_count, p->d_words + kErrWord);
    const msv_status s = launch_forward(p, a, o, n, st);
    return s == MSV_OK ? launch_backward(p, a, o, n, st) : s;
}

msv_status msv_dom_decode_batch(msv_dom_profile* p, const uint8_t* residues, const uint64_t* offsets, uint64_t n,
                                const uint32_t* select, uint64_t n_select, float rt1, float rt2,
                                uint64_t workspace_bytes, msv_dom_result** result) {
    if (!p || !result || (n && !offsets) || (n_select && select && n == 0)) return MSV_ERR_INVALID_ARGUMENT;
    *result = nullptr;
    if (n >= (1ull << 32)) return MSV_ERR_INVALID_ARGUMENT;
    const uint64_t m = select ? n_select : n;
    if (m >= (1ull << 32)) return MSV_ERR_INVALID_ARGUMENT;
    uint64_t longest = 0, total = 0;
    msv_status s = n ? csr_extent(offsets, n, &longest, &total) : MSV_OK;
    if (s != MSV_OK) return s;
    if (total && !residues) return MSV_ERR_INVALID_ARGUMENT;
    std::vector<uint32_t> sel(m);
    for (uint64_t q = 0; q < m; ++q) {
        sel[q] = select ? select[q] : static_cast<uint32_t>(q);
        if (sel[q] >= n) return MSV_ERR_INVALID_ARGUMENT;
    }
    // the chunks, before anything is launched: a sequence that alone exceeds the workspace is refused here
    // (a list with repeats may be longer than the batch, a launch's list may not, seq_queue.h: no chunk over n)
    constexpr uint64_t kRowBytes = domk::kRowWords * sizeof(uint32_t);
    std::vector<uint64_t> bytes(m);
    for (uint64_t q = 0; q < m; ++q) bytes[q] = msv_host::dom_sequence_bytes(offsets[sel[q] + 1] - offsets[sel[q]]);
    itemplan::ChunkLayout lay;  // in record rows
    if (!itemplan::chunk_layout(bytes.data(), m, workspace_bytes, kRowBytes, n, &lay)) return MSV_ERR_OUT_OF_MEMORY;
    const std::vector<uint64_t>&cuts = lay.cuts, &rows = lay.base;
    const std::vector<uint32_t>& counts = lay.counts;
    const uint64_t n_chunks = lay.chunks();
    std::unique_ptr<msv_dom_result> guard(new (std::nothrow) msv_dom_result);
    msv_dom_result* const r = guard.get();
    if (!r) return MSV_ERR_OUT_OF_MEMORY;
    r->stats.chunks = n_chunks;
    r->stats.record_bytes = lay.total_units * kRowBytes;
    r->fwd.assign(m, 0.0f);
    r->bck.assign(m, 0.0f);
    r->res_off.assign(m + 1, 0);
    r->reg_off.assign(m + 1, 0);
    for (uint64_t q = 0; q < m; ++q) r->res_off[q + 1] = r->res_off[q] + (offsets[sel[q] + 1] - offsets[sel[q]]);
    r->begin.assign(r->res_off[m], 0.0f);
    r->end.assign(r->res_off[m], 0.0f);
    r->occ.assign(r->res_off[m], 0.0f);
    if (m == 0) {
        *result = guard.release();
        return MSV_OK;
    }

    DeviceGuard g(p->device);
    if (!g.ok) return MSV_ERR_NO_DEVICE;
    if ((s = msv_dom_profile_reserve_length(p, longest)) != MSV_OK) return s;
    hipStream_t st = p->stream;
    msvrt::CsrStaging& sg = p->staged;
    MSV_HIP(sg.d_scores.reserve(n));
    MSV_HIP(p->d_bck.reserve(n));
    MSV_HIP(p->d_begin.reserve(total));
    MSV_HIP(p->d_end.reserve(total));
    MSV_HIP(p->d_occ.reserve(total));
    MSV_HIP(p->d_records.reserve(lay.chunk_units * domk::kRowWords));
    MSV_HIP(p->d_sel.reserve(m));
    MSV_HIP(p->d_rows.reserve(m));
    MSV_HIP(p->d_counts.reserve(n_chunks));
    MSV_HIP(p->d_rcount.reserve(m));
    MSV_HIP(p->d_roff.reserve(m + 1));
    msvrt::Event ev[4];
    for (auto& e : ev) MSV_HIP(e.create(hipEventDefault));
    msvrt::StreamDrain drain(st);
    MSV_HIP(sg.upload(residues, offsets, 0, n, true, st, st));
    MSV_HIP(hipMemcpyAsync(p->d_sel, sel.data(), m * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    MSV_HIP(hipMemcpyAsync(p->d_rows, rows.data(), m * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    MSV_HIP(hipMemcpyAsync(p->d_counts, counts.data(), n_chunks * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    // an entry the kernels refuse keeps what is set here: NaN scores, zero posteriors
    MSV_HIP(fill_nan(sg.d_scores, n, st));
    MSV_HIP(fill_nan(p->d_bck, n, st));
    if (total) {
        MSV_HIP(hipMemsetAsync(p->d_begin, 0, total * sizeof(float), st));
        MSV_HIP(hipMemsetAsync(p->d_end, 0, total * sizeof(float), st));
        MSV_HIP(hipMemsetAsync(p->d_occ, 0, total * sizeof(float), st));
    }
    Outputs o;
    o.fwd = sg.d_scores;
    o.bck = p->d_bck;
    o.begin = p->d_begin;
    o.end = p->d_end;
    o.occ = p->d_occ;
    o.records = p->d_records;
    uint32_t* const errors = p->d_words + kHostErrWord;
    for (uint64_t c = 0; c < n_chunks; ++c) {
        // the chunk's part of the list, its length in a device word; the offsets are the staged batch's (from 0)
        const domk::DomArgs a =
            batch_args(p, sg.d_res, sg.d_off, n, p->d_sel + cuts[c], p->d_counts + c, errors);
        o.item_rows = p->d_rows + cuts[c];
        MSV_HIP(hipEventRecord(ev[0], st));
        if ((s = launch_forward(p, a, o, counts[c], st)) != MSV_OK) return s;
        MSV_HIP(hipEventRecord(ev[1], st));
        if ((s = launch_backward(p, a, o, counts[c], st)) != MSV_OK) return s;
        MSV_HIP(hipEventRecord(ev[2], st));
        MSV_HIP(hipStreamSynchronize(st));  // the next chunk rewrites the records; the times are read per chunk
        r->stats.forward_ms += elapsed(ev[0], ev[1]);
        r->stats.backward_ms += elapsed(ev[1], ev[2]);
    }
    // the envelope rule over the whole list: count, exclusive scan, place
    domk::RegionArgs ra{};
    ra.offsets = sg.d_off;
    ra.select = p->d_sel;
    ra.fwd_scores = sg.d_scores;
    ra.begin = p->d_begin;
    ra.end = p->d_end;
    ra.occ = p->d_occ;
    ra.n = n;
    ra.m = m;
    ra.rt1 = rt1;
    ra.rt2 = rt2;
    MSV_HIP(hipEventRecord(ev[0], st));
    MSV_HIP(domk::launch_regions_count(ra, p->d_rcount, st));
    MSV_HIP(domk::launch_regions_scan(p->d_rcount, m, p->d_roff, st));
    MSV_HIP(hipMemcpyAsync(r->reg_off.data(), p->d_roff, (m + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    MSV_HIP(hipStreamSynchronize(st));
    const uint64_t n_regions = r->reg_off[m];
    r->regions.resize(n_regions);
    MSV_HIP(p->d_regions.reserve(n_regions));
    MSV_HIP(domk::launch_regions_place(ra, p->d_roff, p->d_regions, st));
    MSV_HIP(hipEventRecord(ev[3], st));
    if (n_regions)
        MSV_HIP(hipMemcpyAsync(r->regions.data(), p->d_regions, n_regions * sizeof(msv_dom_region),
                               hipMemcpyDeviceToHost, st));
    std::vector<float> fwd(n), bck(n), b(total), e(total), oc(total);
    MSV_HIP(hipMemcpyAsync(fwd.data(), sg.d_scores, n * sizeof(float), hipMemcpyDeviceToHost, st));
    MSV_HIP(hipMemcpyAsync(bck.data(), p->d_bck, n * sizeof(float), hipMemcpyDeviceToHost, st));
    if (total) {
        MSV_HIP(hipMemcpyAsync(b.data(), p->d_begin, total * sizeof(float), hipMemcpyDeviceToHost, st));
        MSV_HIP(hipMemcpyAsync(e.data(), p->d_end, total * sizeof(float), hipMemcpyDeviceToHost, st));
        MSV_HIP(hipMemcpyAsync(oc.data(), p->d_occ, total * sizeof(float), hipMemcpyDeviceToHost, st));
    }
    MSV_HIP(hipStreamSynchronize(st));
    drain.disarm();
    r->stats.regions_ms = elapsed(ev[0], ev[3]);
    // compacted per select entry, in the caller's order
    for (uint64_t q = 0; q < m; ++q) {
        const uint64_t o0 = offsets[sel[q]] - offsets[0], L = r->res_off[q + 1] - r->res_off[q];
        r->fwd[q] = fwd[sel[q]];
        r->bck[q] = bck[sel[q]];
        std::copy(b.begin() + o0, b.begin() + o0 + L, r->begin.begin() + r->res_off[q]);
        std::copy(e.begin() + o0, e.begin() + o0 + L, r->end.begin() + r->res_off[q]);
        std::copy(oc.begin() + o0, oc.begin() + o0 + L, r->occ.begin() + r->res_off[q]);
    }
    s = stagedev::read_errors(p, kHostErrWord, st);
    if (s != MSV_OK && s != MSV_ERR_BAD_RESIDUE && s != MSV_ERR_SEQUENCE_TOO_LONG) return s;
    *result = guard.release();
    return s;
}

uint64_t msv_dom_result_count(const msv_dom_result* r) { return r ? r->fwd.size() : 0; }
uint64_t msv_dom_result_residues(const msv_dom_result* r) { return r ? r->begin.size() : 0; }
uint64_t msv_dom_result_regions(const msv_dom_result* r) { return r ? r->regions.size() : 0; }

msv_status msv_dom_result_copy(const msv_dom_result* r, float* fwd_scores, float* bck_scores,
                               uint64_t* residue_offsets, float* begin, float* end, float* occ,
                               uint64_t* region_offsets, msv_dom_region* regions) {
    if (!r) return MSV_ERR_INVALID_ARGUMENT;
    if (fwd_scores) std::copy(r->fwd.begin(), r->fwd.end(), fwd_scores);
    if (bck_scores) std::copy(r->bck.begin(), r->bck.end(), bck_scores);
    if (residue_offsets) std::copy(r->res_off.begin(), r->res_off.end(), residue_offsets);
    if (begin) std::copy(r->begin.begin(), r->begin.end(), begin);
    if (end) std::copy(r->end.begin(), r->end.end(), end);
    if (occ) std::copy(r->occ.begin(), r->occ.end(), occ);
    if (region_offsets) std::copy(r->reg_off.begin(), r->reg_off.end(), region_offsets);
    if (regions) std::copy(r->regions.begin(), r->regions.end(), regions);
    return MSV_OK;
}

void msv_dom_result_free(msv_dom_result* r) { delete r; }

msv_status msv_dom_result_stats(const msv_dom_result* r, msv_dom_stats* out) {
    if (!r || !out) return MSV_ERR_INVALID_ARGUMENT;
    *out = r->stats;
    return MSV_OK;
}

}  // extern "C"
