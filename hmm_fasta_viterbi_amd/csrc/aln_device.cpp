// aln_device.cpp -- C-ABI of the alignment stage (msv.h) on the HIP runtime.
//
// The stage runs on a msv_dom_profile (dom_profile.h): the recording and the Backward kernel of aln_kernel.hip read
// the tables the domain stage's variant installed, the fill kernel a small table of gate bytes made per call.  The
// item checks, the items' residues packed into a CSR batch of their own (item q is sequence q of it) and the chunks
// that fit the workspace are item_plan.h's, shared with the split stage; this file allocates the result, adds the
// null2 unit lists and runs five launches per chunk, the first three each on its own launch slot (stagedev::run with
// the kernel's own grid): recording Forward, Backward with the combine, OA fill, walk count, walk place.  With the
// null2 option two more, plain launches of aln_null2.hip that only read the workspace, after the count
// walk: the row-block partial sums into a slab buffer of the call's own, then one wave per item that finishes
// null2[20].
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <new>
#include <vector>

#include "aln_host.h"
#include "aln_kernel.h"
#include "aln_null2.h"
#include "dom_profile.h"
#include "hip_rt.h"
#include "host_cpu.h"
#include "msv.h"
#include "msv_kernel.h"
#include "null2_host.h"
#include "stage_profile.h"

using msvrt::DeviceBuffer;
using msvrt::DeviceGuard;
using stagedev::kHostErrWord;

struct msv_aln_result {
    std::vector<float> env, oa;
    std::vector<uint64_t> dom_off;
    std::vector<msv_vit_domain> domains;
    std::vector<uint8_t> ops;
    std::vector<float> op_pp;
    // keep_posteriors: per item, ppM / ppI [Le][M] and ppN / ppJ / ppC [Le]
    bool kept = false;
    uint32_t M = 0;
    std::vector<std::vector<float>> pm, pi, pn, pj, pc;
    msv_aln_stats stats{};
    // the null2 option: per item null2 [20] and the correction (zeros where the item was not decoded)
    bool has_null2 = false;
    std::vector<float> null2, domcorr;
    float null2_ms = 0.0f, null2_partial_ms = 0.0f;
    uint64_t slab_bytes = 0;
};

namespace {

using itemplan::kDefaultWorkspace;
using msv_host::read_sized;
using msv_host::write_sized;
using msvrt::elapsed;
using msvrt::fill_nan;
using msvrt::kernel_footprint;
using msvrt::upload;

const alnk::AlnVariant* variant_of(const msv_dom_profile* p) {
    return stagedev::find_by_shape(alnk::aln_variants, p->v->S, p->v->isc);
}

// One persistent launch on the next launch slot over `items` list entries, `waves` of them a workgroup.
msv_status run_kernel(msv_dom_profile* p, const void* fn, int waves, hipStream_t st, uint64_t items, alnk::AlnArgs& a) {
    return stagedev::run(p, st, items, static_cast<uint64_t>(waves), msvrt::full_grid(p->device, fn, waves * 64),
                         [&](uint32_t blocks, uint32_t* counter) {
                             a.counter = counter;
                             return alnk::aln_launch(fn, waves, blocks, a, st);
                         });
}

msv_status align_batch(msv_dom_profile* p, const uint8_t* residues, const uint64_t* offsets, uint64_t n,
                       const msv_aln_item* items, uint64_t m, uint64_t workspace_bytes, int keep_posteriors,
                       bool null2, msv_aln_result** result) {
    if (!p || !result || (n && !offsets) || (m && !items)) return MSV_ERR_INVALID_ARGUMENT;
    *result = nullptr;
    uint64_t longest = 0;
    msv_status s = itemplan::check_items(residues, offsets, n, items, m, &longest);
    if (s != MSV_OK) return s;
    const alnk::AlnVariant* v = variant_of(p);
    if (!v) return MSV_ERR_UNSUPPORTED_MODEL;
    const uint64_t S = static_cast<uint64_t>(v->S);
    const uint32_t M = p->model_length, K = M - 1;

    std::unique_ptr<msv_aln_result> guard(new (std::nothrow) msv_aln_result);
    msv_aln_result* const r = guard.get();
    if (!r) return MSV_ERR_OUT_OF_MEMORY;
    r->M = M;
    r->kept = keep_posteriors != 0;
    r->has_null2 = null2;
    if (null2) {
        r->null2.assign(m * msv_host::kNull2Residues, 0.0f);
        r->domcorr.assign(m, 0.0f);
    }
    r->env.assign(m, std::nanf(""));
    r->oa.assign(m, std::nanf(""));
    r->dom_off.assign(m + 1, 0);
    if (r->kept) {
        r->pm.resize(m), r->pi.resize(m), r->pn.resize(m), r->pj.resize(m), r->pc.resize(m);
    }
    auto give = [&](msv_status st) {
        *result = guard.release();
        return st;
    };
    if (m == 0) return give(MSV_OK);

    // the items as a batch of their own, and the chunks, before anything is launched (item_plan.h)
    itemplan::ItemBatch plan;
    if (!itemplan::plan_items(residues, offsets, items, m, workspace_bytes,
                              [S](uint64_t Le) { return msv_host::aln_item_bytes(S, Le); }, &plan))
        return give(MSV_ERR_OUT_OF_MEMORY);  // (nothing launched: the result says so, chunks = 0)
    const std::vector<uint64_t>&poff = plan.poff, &bytes = plan.bytes, &cuts = plan.lay.cuts, &base = plan.lay.base;
    const std::vector<uint32_t>&lc = plan.lc, &sel = plan.sel, &counts = plan.lay.counts;
    const std::vector<uint8_t>& packed = plan.packed;
    const uint64_t n_chunks = plan.lay.chunks(), chunk_words = plan.lay.chunk_units;
    // null2: the units (item, block of kNull2RowBlock rows) of every chunk, chunk after chunk
    const alnk::Null2Variant* nv = null2 ? alnk::null2_variant(v->S, v->isc) : nullptr;
    if (null2 && !nv) return MSV_ERR_UNSUPPORTED_MODEL;
    std::vector<uint32_t> unit_item, unit_first;
    std::vector<uint64_t> unit_start;
    uint64_t chunk_units = 0;
    if (null2) {
        unit_first.resize(m);
        unit_start.assign(n_chunks + 1, 0);
        for (uint64_t c = 0; c < n_chunks; ++c) {
            uint64_t at = 0;
            for (uint64_t q = cuts[c]; q < cuts[c + 1]; ++q) {
                const uint64_t nb = msv_host::null2_blocks(poff[q + 1] - poff[q]);
                if (at + nb >= (1ull << 32)) return give(MSV_ERR_OUT_OF_MEMORY);
                unit_first[q] = static_cast<uint32_t>(at);
                unit_item.insert(unit_item.end(), nb, static_cast<uint32_t>(q));
                at += nb;
            }
            unit_start[c + 1] = unit_start[c] + at;
            chunk_units = std::max(chunk_units, at);
        }
    }

    DeviceGuard g(p->device);
    if (!g.ok) return MSV_ERR_NO_DEVICE;
    if ((s = msv_dom_profile_reserve_length(p, longest)) != MSV_OK) return s;
    hipStream_t st = p->stream;
    msvrt::CsrStaging& sg = p->staged;
    const std::vector<uint32_t> gates =
        msv_host::aln_gates(p->tsc.data(), M, p->tr_B_Mk, v->S);
    DeviceBuffer<uint32_t> d_ws, d_lc, d_sel, d_counts, d_gates, d_wcounts;
    DeviceBuffer<uint64_t> d_base, d_domoff, d_opsoff;
    DeviceBuffer<float> d_oa, d_oppp;
    DeviceBuffer<msv_aln_item> d_items;
    DeviceBuffer<msv_vit_domain> d_doms;
    DeviceBuffer<uint8_t> d_ops;
    DeviceBuffer<uint32_t> d_unit_item, d_unit_first;
    DeviceBuffer<float> d_slabs, d_null2;
    msvrt::Event ev[8], ev_null2, ev_null2_mid;
    for (auto& e : ev) MSV_HIP(e.create(hipEventDefault));
    if (null2) {
        // the slabs are the call's own, about 1 / kNull2RowBlock of the matrix: never the caller's workspace
        MSV_HIP(ev_null2.create(hipEventDefault));
        MSV_HIP(ev_null2_mid.create(hipEventDefault));
        MSV_HIP(d_slabs.reserve(chunk_units * msv_host::null2_slab_floats(S)));
        MSV_HIP(d_null2.reserve(m * msv_host::kNull2Residues));
        r->slab_bytes = chunk_units * msv_host::null2_slab_floats(S) * sizeof(float);
    }
    MSV_HIP(sg.d_scores.reserve(m));
    MSV_HIP(d_oa.reserve(m));
    MSV_HIP(d_ws.reserve(chunk_words));
    MSV_HIP(d_wcounts.reserve(2 * plan.lay.chunk_entries));
    msvrt::StreamDrain drain(st);
    MSV_HIP(sg.upload(packed.data(), poff.data(), 0, m, true, st, st));
    MSV_HIP(upload(d_lc, lc, st));
    MSV_HIP(upload(d_sel, sel, st));
    MSV_HIP(upload(d_counts, counts, st));
    MSV_HIP(upload(d_gates, gates, st));
    MSV_HIP(upload(d_base, base, st));
    MSV_HIP(d_items.reserve(m));
    MSV_HIP(hipMemcpyAsync(d_items, items, m * sizeof(msv_aln_item), hipMemcpyHostToDevice, st));
    // an item the kernels refuse keeps what is set here: NaN scores
    MSV_HIP(fill_nan(sg.d_scores, m, st));
    MSV_HIP(fill_nan(d_oa, m, st));
    alnk::Null2Args na{};
    if (null2) {
        MSV_HIP(upload(d_unit_item, unit_item, st));
        MSV_HIP(upload(d_unit_first, unit_first, st));
        // an item the kernels skip keeps what is set here: zeros
        MSV_HIP(hipMemsetAsync(d_null2, 0, m * msv_host::kNull2Residues * sizeof(float), st));
        na.ws = d_ws;
        na.base = d_base;
        na.offsets = sg.d_off;
        na.scores = sg.d_scores;
        na.unit_first = d_unit_first;
        na.slabs = d_slabs;
        na.etab = p->d_etab;
        na.itab = p->d_itab ? p->d_itab.get() : p->d_etab.get();
        na.null2 = d_null2;
        na.leng = K;
    }

    alnk::AlnArgs a{};
    a.etab = p->d_etab;
    a.itab = p->d_itab ? p->d_itab.get() : p->d_etab.get();
    a.gates = d_gates;
    a.residues = sg.d_res;
    a.offsets = sg.d_off;
    a.lc = d_lc;
    a.base = d_base;
    a.lentab = p->d_lentab;
    a.scores = sg.d_scores;
    a.oa_scores = d_oa;
    a.ws = d_ws;
    a.errors = p->d_words + kHostErrWord;
    a.n = m;
    a.lentab_n = p->lentab_n;
    a.tBM = p->tBM;
    a.tEC = p->tEC;
    a.tEJ = p->tEJ;
    a.open_EC = std::isfinite(p->tr_E_C) ? 1u : 0u;
    a.open_EJ = std::isfinite(p->tr_E_J) ? 1u : 0u;

    std::vector<uint32_t> wc;
    std::vector<uint64_t> doff, ooff;
    std::vector<uint32_t> host_ws;
    std::vector<msv_vit_domain> cdoms;
    for (uint64_t c = 0; c < n_chunks; ++c) {
        const uint64_t lo = cuts[c], hi = cuts[c + 1], cnt = hi - lo;
        a.select = d_sel + lo;
        a.select_count = d_counts + c;
        MSV_HIP(hipEventRecord(ev[0], st));
        a.ttab = p->d_ttab;
        a.scan = p->d_scan;
        if ((s = run_kernel(p, v->fwd_fn, v->waves, st, cnt, a)) != MSV_OK) return s;
        MSV_HIP(hipEventRecord(ev[1], st));
        a.ttab = p->d_btab;
        a.scan = p->d_bscan;
        if ((s = run_kernel(p, v->bck_fn, v->waves, st, cnt, a)) != MSV_OK) return s;
        MSV_HIP(hipEventRecord(ev[2], st));
        if ((s = run_kernel(p, v->fill_fn, alnk::kFillWaves, st, cnt, a)) != MSV_OK) return s;
        MSV_HIP(hipEventRecord(ev[3], st));
        alnk::WalkArgs w{};
        w.ws = d_ws;
        w.base = d_base;
        w.offsets = sg.d_off;
        w.scores = sg.d_scores;
        w.oa_scores = d_oa;
        w.items = d_items;
        w.lo = static_cast<uint32_t>(lo);
        w.hi = static_cast<uint32_t>(hi);
        w.S = static_cast<uint32_t>(S);
        w.counts = d_wcounts;
        MSV_HIP(alnk::launch_walk(w, st));
        MSV_HIP(hipEventRecord(ev[4], st));
        if (null2) {  // behind the count walk, so that the four existing launch kinds keep their own event pairs
            na.unit_item = d_unit_item + unit_start[c];
            na.units = static_cast<uint32_t>(unit_start[c + 1] - unit_start[c]);
            na.lo = static_cast<uint32_t>(lo);
            na.hi = static_cast<uint32_t>(hi);
            MSV_HIP(alnk::null2_launch_partial(nv, na, st));
            MSV_HIP(hipEventRecord(ev_null2_mid, st));
            MSV_HIP(alnk::null2_launch_finish(nv, na, st));
            MSV_HIP(hipEventRecord(ev_null2, st));
        }
        wc.assign(2 * cnt, 0);
        MSV_HIP(hipMemcpyAsync(wc.data(), d_wcounts, 2 * cnt * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        MSV_HIP(hipStreamSynchronize(st));
        doff.assign(cnt + 1, 0);
        ooff.assign(cnt + 1, 0);
        for (uint64_t j = 0; j < cnt; ++j) {
            doff[j + 1] = doff[j] + wc[2 * j];
            ooff[j + 1] = ooff[j] + wc[2 * j + 1];
        }
        const uint64_t nd = doff[cnt], no = ooff[cnt];
        const uint64_t ops0 = r->ops.size(), dom0 = r->domains.size();
        MSV_HIP(upload(d_domoff, doff, st));
        MSV_HIP(upload(d_opsoff, ooff, st));
        MSV_HIP(d_doms.reserve(nd));
        MSV_HIP(d_ops.reserve(no));
        MSV_HIP(d_oppp.reserve(no));
        w.dom_off = d_domoff;
        w.ops_off = d_opsoff;
        w.domains = d_doms;
        w.ops = d_ops;
        w.op_pp = d_oppp;
        MSV_HIP(hipEventRecord(ev[5], st));
        if (nd) MSV_HIP(alnk::launch_walk(w, st));
        MSV_HIP(hipEventRecord(ev[6], st));
        r->domains.resize(dom0 + nd);
        r->ops.resize(ops0 + no);
        r->op_pp.resize(ops0 + no);
        if (nd) {
            MSV_HIP(hipMemcpyAsync(r->domains.data() + dom0, d_doms, nd * sizeof(msv_vit_domain), hipMemcpyDeviceToHost,
                                   st));
            MSV_HIP(hipMemcpyAsync(r->ops.data() + ops0, d_ops, no, hipMemcpyDeviceToHost, st));
            MSV_HIP(hipMemcpyAsync(r->op_pp.data() + ops0, d_oppp, no * sizeof(float), hipMemcpyDeviceToHost, st));
        }
        uint64_t words = 0;
        for (uint64_t q = lo; q < hi; ++q) words += bytes[q] / 4;
        if (r->kept) {
            host_ws.resize(words);
            MSV_HIP(hipMemcpyAsync(host_ws.data(), d_ws, words * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        }
        MSV_HIP(hipMemcpyAsync(r->env.data() + lo, sg.d_scores + lo, cnt * sizeof(float), hipMemcpyDeviceToHost, st));
        MSV_HIP(hipMemcpyAsync(r->oa.data() + lo, d_oa + lo, cnt * sizeof(float), hipMemcpyDeviceToHost, st));
        MSV_HIP(hipStreamSynchronize(st));  // the next chunk rewrites the workspace; the times are read per chunk
        r->stats.forward_ms += elapsed(ev[0], ev[1]);
        r->stats.backward_ms += elapsed(ev[1], ev[2]);
        r->stats.fill_ms += elapsed(ev[2], ev[3]);
        r->stats.walk_ms += elapsed(ev[3], ev[4]) + elapsed(ev[5], ev[6]);
        r->stats.chunks += 1;
        if (null2) {
            r->null2_ms += elapsed(ev[4], ev_null2);
            r->null2_partial_ms += elapsed(ev[4], ev_null2_mid);
        }
        for (uint64_t j = 0; j < cnt; ++j) {
            r->dom_off[lo + j + 1] = dom0 + doff[j + 1];
            r->stats.matrix_bytes += 4 * msv_host::aln_matrix_words(S, poff[lo + j + 1] - poff[lo + j]);
        }
        for (uint64_t d = dom0; d < dom0 + nd; ++d) r->domains[d].ops_begin += ops0;
        if (r->kept)
            for (uint64_t q = lo; q < hi; ++q) {
                const uint64_t Le = poff[q + 1] - poff[q];
                r->pm[q].assign(Le * M, 0.0f);
                r->pi[q].assign(Le * M, 0.0f);
                r->pn[q].assign(Le, 0.0f);
                r->pj[q].assign(Le, 0.0f);
                r->pc[q].assign(Le, 0.0f);
                if (!std::isfinite(r->env[q])) continue;
                const uint32_t* rec = host_ws.data() + base[q];
                const float* mat = reinterpret_cast<const float*>(rec + msv_host::aln_record_words(Le));
                for (uint64_t i = 0; i < Le; ++i) {
                    std::memcpy(&r->pn[q][i], rec + (i + 1) * 6 + 0, 4);
                    std::memcpy(&r->pj[q][i], rec + (i + 1) * 6 + 1, 4);
                    std::memcpy(&r->pc[q][i], rec + (i + 1) * 6 + 2, 4);
                    const float* row = mat + i * 2 * S * 64;
                    for (uint32_t k = 1; k <= K; ++k) {
                        const uint64_t l = (k - 1) / S, sl = (k - 1) % S;
                        r->pm[q][i * M + k] = row[sl * 64 + l];
                        r->pi[q][i * M + k] = row[(S + sl) * 64 + l];
                    }
                }
            }
    }
    if (null2) {
        MSV_HIP(hipMemcpyAsync(r->null2.data(), d_null2, r->null2.size() * sizeof(float), hipMemcpyDeviceToHost, st));
        MSV_HIP(hipStreamSynchronize(st));
        // THE definition of the correction, on the device's own null2: the device's domcorrection has its bits
        for (uint64_t q = 0; q < m; ++q)
            if (std::isfinite(r->env[q]))
                r->domcorr[q] = msv_host::null2_correction(r->null2.data() + q * msv_host::kNull2Residues,
                                                           packed.data() + poff[q], poff[q + 1] - poff[q]);
    }
    drain.disarm();
    s = stagedev::read_errors(p, kHostErrWord, st);
    if (s != MSV_OK && s != MSV_ERR_BAD_RESIDUE && s != MSV_ERR_SEQUENCE_TOO_LONG) return s;
    return give(s);
}

}  // namespace

extern "C" {

msv_status msv_aln_align_batch_opts(msv_dom_profile* p, const uint8_t* residues, const uint64_t* offsets, uint64_t n,
                                    const msv_aln_item* items, uint64_t m, const msv_aln_options* options,
                                    msv_aln_result** result) {
    msv_aln_options o;
    if (!read_sized(options, &o, sizeof(uint64_t))) return MSV_ERR_INVALID_ARGUMENT;
    return align_batch(p, residues, offsets, n, items, m, o.workspace_bytes, o.keep_posteriors, o.null2 != 0, result);
}

msv_status msv_aln_align_batch(msv_dom_profile* p, const uint8_t* residues, const uint64_t* offsets, uint64_t n,
                               const msv_aln_item* items, uint64_t m, uint64_t workspace_bytes, int keep_posteriors,
                               msv_aln_result** result) {
    msv_aln_options o;
    std::memset(&o, 0, sizeof(o));
    o.struct_size = sizeof(o);
    o.workspace_bytes = workspace_bytes;
    o.keep_posteriors = keep_posteriors;
    return msv_aln_align_batch_opts(p, residues, offsets, n, items, m, &o, result);
}

msv_status msv_aln_result_null2(const msv_aln_result* r, float* null2, float* domcorrection) {
    if (!r || !r->has_null2) return MSV_ERR_INVALID_ARGUMENT;
    if (null2) std::copy(r->null2.begin(), r->null2.end(), null2);
    if (domcorrection) std::copy(r->domcorr.begin(), r->domcorr.end(), domcorrection);
    return MSV_OK;
}

msv_status msv_aln_result_null2_stats(const msv_aln_result* r, msv_aln_null2_stats* out) {
    if (!r || !out || !r->has_null2 || out->struct_size < sizeof(uint32_t)) return MSV_ERR_INVALID_ARGUMENT;
    msv_aln_null2_stats st;
    std::memset(&st, 0, sizeof(st));
    st.row_block = static_cast<uint32_t>(msv_host::kNull2RowBlock);
    st.null2_ms = r->null2_ms;
    st.partial_ms = r->null2_partial_ms;
    st.slab_bytes = r->slab_bytes;
    write_sized(out, st);
    return MSV_OK;
}

uint64_t msv_aln_result_count(const msv_aln_result* r) { return r ? r->env.size() : 0; }
uint64_t msv_aln_result_domains(const msv_aln_result* r) { return r ? r->domains.size() : 0; }
uint64_t msv_aln_result_ops(const msv_aln_result* r) { return r ? r->ops.size() : 0; }

msv_status msv_aln_result_copy(const msv_aln_result* r, float* envelope_scores, float* oa_scores,
                               uint64_t* domain_offsets, msv_vit_domain* domains, uint8_t* ops, float* op_pp) {
    if (!r) return MSV_ERR_INVALID_ARGUMENT;
    if (envelope_scores) std::copy(r->env.begin(), r->env.end(), envelope_scores);
    if (oa_scores) std::copy(r->oa.begin(), r->oa.end(), oa_scores);
    if (domain_offsets) std::copy(r->dom_off.begin(), r->dom_off.end(), domain_offsets);
    if (domains) std::copy(r->domains.begin(), r->domains.end(), domains);
    if (ops) std::copy(r->ops.begin(), r->ops.end(), ops);
    if (op_pp) std::copy(r->op_pp.begin(), r->op_pp.end(), op_pp);
    return MSV_OK;
}

msv_status msv_aln_result_posteriors(const msv_aln_result* r, uint64_t q, float* ppM, float* ppI, float* ppN,
                                     float* ppJ, float* ppC) {
    if (!r || !r->kept || q >= r->pm.size()) return MSV_ERR_INVALID_ARGUMENT;
    if (ppM) std::copy(r->pm[q].begin(), r->pm[q].end(), ppM);
    if (ppI) std::copy(r->pi[q].begin(), r->pi[q].end(), ppI);
    if (ppN) std::copy(r->pn[q].begin(), r->pn[q].end(), ppN);
    if (ppJ) std::copy(r->pj[q].begin(), r->pj[q].end(), ppJ);
    if (ppC) std::copy(r->pc[q].begin(), r->pc[q].end(), ppC);
    return MSV_OK;
}

void msv_aln_result_free(msv_aln_result* r) { delete r; }

msv_status msv_aln_result_stats(const msv_aln_result* r, msv_aln_stats* out) {
    if (!r || !out) return MSV_ERR_INVALID_ARGUMENT;
    *out = r->stats;
    return MSV_OK;
}

msv_status msv_aln_describe(const msv_dom_profile* p, msv_aln_info* out) {
    if (!p || !out || out->struct_size < sizeof(uint32_t)) return MSV_ERR_INVALID_ARGUMENT;
    const alnk::AlnVariant* v = variant_of(p);
    if (!v) return MSV_ERR_UNSUPPORTED_MODEL;
    DeviceGuard g(p->device);
    if (!g.ok) return MSV_ERR_NO_DEVICE;
    msv_aln_info info;
    std::memset(&info, 0, sizeof(info));
    info.states_per_lane = static_cast<uint32_t>(v->S);
    info.pointer_words = static_cast<uint32_t>(msv_host::aln_pointer_words(static_cast<uint64_t>(v->S)));
    info.forward_blocks = msvrt::full_grid(p->device, v->fwd_fn, v->waves * 64);
    info.backward_blocks = msvrt::full_grid(p->device, v->bck_fn, v->waves * 64);
    info.fill_blocks = msvrt::full_grid(p->device, v->fill_fn, alnk::kFillWaves * 64);
    info.default_workspace_bytes = kDefaultWorkspace;
    std::snprintf(info.variant, sizeof(info.variant), "%s", v->name);
    kernel_footprint(v->fwd_fn, &info.forward_scratch_bytes, &info.forward_lds_bytes);
    kernel_footprint(v->bck_fn, &info.backward_scratch_bytes, &info.backward_lds_bytes);
    kernel_footprint(v->fill_fn, &info.fill_scratch_bytes, &info.fill_lds_bytes);
    kernel_footprint(alnk::walk_fn(), &info.walk_scratch_bytes, &info.walk_lds_bytes);
    info.null2_row_block = static_cast<uint32_t>(msv_host::kNull2RowBlock);
    if (const alnk::Null2Variant* nv = alnk::null2_variant(v->S, v->isc)) {
        kernel_footprint(nv->partial_fn, &info.null2_partial_scratch_bytes, &info.null2_partial_lds_bytes);
        kernel_footprint(nv->finish_fn, &info.null2_finish_scratch_bytes, &info.null2_finish_lds_bytes);
    }
    write_sized(out, info);
    return MSV_OK;
}

}  // extern "C"
