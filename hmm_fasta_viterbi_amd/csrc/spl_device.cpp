// spl_device.cpp -- C-ABI of the split stage (msv.h) on the HIP runtime.
//
// The stage runs on a msv_dom_profile as the alignment stage does (aln_device.cpp): the recording kernel of
// spl_kernel.hip reads the tables the domain stage's variant installed, the sampler a flat table of the float32
// transition odds made per call.  The item checks, the items' residues packed into a CSR batch of their own (item q
// is sequence q of it) and the chunks that fit the workspace are item_plan.h's, as the alignment stage's; this file
// allocates the result and runs three launches per chunk: the recording Forward on a launch slot of its own
// (stagedev::run with that kernel's grid), the sampler's count pass and, after a host scan, its place pass.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <new>
#include <vector>

#include "dom_profile.h"
#include "hip_rt.h"
#include "host_cpu.h"
#include "msv.h"
#include "msv_kernel.h"
#include "spl_host.h"
#include "spl_kernel.h"
#include "stage_profile.h"

using msvrt::DeviceBuffer;
using msvrt::DeviceGuard;
using stagedev::kHostErrWord;

struct msv_spl_result {
    std::vector<float> env;
    std::vector<uint64_t> sample_off;  // [m * n_samples + 1]
    std::vector<msv_spl_segment> segments;
    bool kept = false;
    uint32_t M = 0;
    std::vector<std::vector<float>> fm, fi, fd;
    std::vector<std::vector<uint32_t>> rec;
    msv_spl_stats stats{};
};

namespace {

using itemplan::kDefaultWorkspace;
using msv_host::read_sized;
using msv_host::write_sized;
using msvrt::elapsed;
using msvrt::upload;

constexpr uint32_t kDefaultSamples = 200;
constexpr uint64_t kDefaultSeed = 42;

msv_status sample_batch(msv_dom_profile* p, const uint8_t* residues, const uint64_t* offsets, uint64_t n,
                        const msv_aln_item* items, uint64_t m, const msv_spl_options& opt, msv_spl_result** result) {
    if (!p || !result || (n && !offsets) || (m && !items)) return MSV_ERR_INVALID_ARGUMENT;
    *result = nullptr;
    const uint32_t ns = opt.n_samples ? opt.n_samples : kDefaultSamples;
    const uint64_t seed = opt.seed_set ? opt.seed : kDefaultSeed;
    // (every refusal up to here and check_items' first is the same status: m * ns may wrap only where m is refused)
    if (ns >= (1u << 24) || m * ns >= (1ull << 32)) return MSV_ERR_INVALID_ARGUMENT;
    uint64_t longest = 0;
    msv_status s = itemplan::check_items(residues, offsets, n, items, m, &longest);
    if (s != MSV_OK) return s;
    const splk::SplVariant* v = stagedev::find_by_shape(splk::spl_variants, p->v->S, p->v->isc);
    if (!v) return MSV_ERR_UNSUPPORTED_MODEL;
    const uint64_t S = static_cast<uint64_t>(v->S);
    const uint32_t M = p->model_length, K = M - 1;

    std::unique_ptr<msv_spl_result> guard(new (std::nothrow) msv_spl_result);
    msv_spl_result* const r = guard.get();
    if (!r) return MSV_ERR_OUT_OF_MEMORY;
    r->M = M;
    r->kept = opt.keep_matrix != 0;
    r->stats.n_samples = ns;
    r->stats.seed = seed;
    r->env.assign(m, std::nanf(""));
    r->sample_off.assign(m * ns + 1, 0);
    if (r->kept) r->fm.resize(m), r->fi.resize(m), r->fd.resize(m), r->rec.resize(m);
    auto give = [&](msv_status st) {
        *result = guard.release();
        return st;
    };
    if (m == 0) return give(MSV_OK);

    // the items as a batch of their own, and the chunks, before anything is launched (item_plan.h)
    itemplan::ItemBatch plan;
    if (!itemplan::plan_items(residues, offsets, items, m, opt.workspace_bytes,
                              [S](uint64_t Le) { return msv_host::spl_item_bytes(S, Le); }, &plan))
        return give(MSV_ERR_OUT_OF_MEMORY);  // (nothing launched: the result says so, chunks = 0)
    const std::vector<uint64_t>&poff = plan.poff, &bytes = plan.bytes, &cuts = plan.lay.cuts, &base = plan.lay.base;
    const uint64_t n_chunks = plan.lay.chunks();

    DeviceGuard g(p->device);
    if (!g.ok) return MSV_ERR_NO_DEVICE;
    if ((s = msv_dom_profile_reserve_length(p, longest)) != MSV_OK) return s;
    hipStream_t st = stagedev::stream_of(p, opt.stream);
    msvrt::CsrStaging& sg = p->staged;
    const std::vector<float> tr = msv_host::spl_odds(p->tsc.data(), M);
    DeviceBuffer<uint32_t> d_ws, d_lc, d_sel, d_counts, d_scounts;
    DeviceBuffer<uint64_t> d_base, d_segoff;
    DeviceBuffer<float> d_tr;
    DeviceBuffer<msv_aln_item> d_items;
    DeviceBuffer<msv_spl_segment> d_segs;
    msvrt::Event ev[5];
    for (auto& e : ev) MSV_HIP(e.create(hipEventDefault));
    MSV_HIP(sg.d_scores.reserve(m));
    MSV_HIP(d_ws.reserve(plan.lay.chunk_units));
    MSV_HIP(d_scounts.reserve(plan.lay.chunk_entries * ns));
    msvrt::StreamDrain drain(st);
    MSV_HIP(sg.upload(plan.packed.data(), poff.data(), 0, m, true, st, st));
    MSV_HIP(upload(d_lc, plan.lc, st));
    MSV_HIP(upload(d_sel, plan.sel, st));
    MSV_HIP(upload(d_counts, plan.lay.counts, st));
    MSV_HIP(upload(d_base, base, st));
    MSV_HIP(upload(d_tr, tr, st));
    MSV_HIP(d_items.reserve(m));
    MSV_HIP(hipMemcpyAsync(d_items, items, m * sizeof(msv_aln_item), hipMemcpyHostToDevice, st));
    // an item the kernel refuses keeps what is set here: a NaN score
    MSV_HIP(msvrt::fill_nan(sg.d_scores, m, st));

    splk::SplArgs a{};
    a.etab = p->d_etab;
    a.itab = p->d_itab ? p->d_itab.get() : p->d_etab.get();
    a.ttab = p->d_ttab;
    a.scan = p->d_scan;
    a.residues = sg.d_res;
    a.offsets = sg.d_off;
    a.lc = d_lc;
    a.base = d_base;
    a.lentab = p->d_lentab;
    a.scores = sg.d_scores;
    a.ws = d_ws;
    a.errors = p->d_words + kHostErrWord;
    a.n = m;
    a.lentab_n = p->lentab_n;
    a.tBM = p->tBM;
    a.tEC = p->tEC;
    a.tEJ = p->tEJ;

    splk::SampleArgs w{};
    w.ws = d_ws;
    w.base = d_base;
    w.offsets = sg.d_off;
    w.scores = sg.d_scores;
    w.items = d_items;
    w.lc = d_lc;
    w.lentab = p->d_lentab;
    w.tr = d_tr;
    w.S = static_cast<uint32_t>(S);
    w.leng = K;
    w.n_samples = ns;
    w.tBM = p->tBM;
    w.tEC = p->tEC;
    w.tEJ = p->tEJ;
    w.seed = seed;

    std::vector<uint32_t> sc;
    std::vector<uint64_t> soff;
    std::vector<uint32_t> host_ws;
    for (uint64_t c = 0; c < n_chunks; ++c) {
        const uint64_t lo = cuts[c], hi = cuts[c + 1], cnt = hi - lo;
        a.select = d_sel + lo;
        a.select_count = d_counts + c;
        MSV_HIP(hipEventRecord(ev[0], st));
        s = stagedev::run(p, st, cnt, static_cast<uint64_t>(v->waves),
                          msvrt::full_grid(p->device, v->fwd_fn, v->waves * 64),
                          [&](uint32_t blocks, uint32_t* counter) {
                              a.counter = counter;
                              return splk::spl_launch(v->fwd_fn, v->waves, blocks, a, st);
                          });
        if (s != MSV_OK) return s;
        MSV_HIP(hipEventRecord(ev[1], st));
        w.lo = static_cast<uint32_t>(lo);
        w.hi = static_cast<uint32_t>(hi);
        w.counts = d_scounts;
        w.seg_off = nullptr;
        w.segments = nullptr;
        MSV_HIP(splk::launch_sample(w, st));
        MSV_HIP(hipEventRecord(ev[2], st));
        sc.assign(cnt * ns, 0);
        MSV_HIP(hipMemcpyAsync(sc.data(), d_scounts, cnt * ns * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        MSV_HIP(hipStreamSynchronize(st));
        soff.assign(cnt * ns + 1, 0);
        for (uint64_t j = 0; j < cnt * ns; ++j) {
            soff[j + 1] = soff[j] + (sc[j] & 0x7fffffffu);
            r->stats.truncated += sc[j] >> 31;
        }
        const uint64_t nseg = soff[cnt * ns], seg0 = r->segments.size();
        MSV_HIP(upload(d_segoff, soff, st));
        MSV_HIP(d_segs.reserve(nseg));
        w.seg_off = d_segoff;
        w.segments = d_segs;
        MSV_HIP(hipEventRecord(ev[3], st));
        if (nseg) MSV_HIP(splk::launch_sample(w, st));
        MSV_HIP(hipEventRecord(ev[4], st));
        r->segments.resize(seg0 + nseg);
        if (nseg)
            MSV_HIP(hipMemcpyAsync(r->segments.data() + seg0, d_segs, nseg * sizeof(msv_spl_segment),
                                   hipMemcpyDeviceToHost, st));
        uint64_t words = 0;
        for (uint64_t q = lo; q < hi; ++q) words += bytes[q] / 4;
        if (r->kept) {
            host_ws.resize(words);
            MSV_HIP(hipMemcpyAsync(host_ws.data(), d_ws, words * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        }
        MSV_HIP(hipMemcpyAsync(r->env.data() + lo, sg.d_scores + lo, cnt * sizeof(float), hipMemcpyDeviceToHost, st));
        MSV_HIP(hipStreamSynchronize(st));  // the next chunk rewrites the workspace; the times are read per chunk
        r->stats.forward_ms += elapsed(ev[0], ev[1]);
        r->stats.sample_ms += elapsed(ev[1], ev[2]) + elapsed(ev[3], ev[4]);
        r->stats.chunks += 1;
        for (uint64_t j = 0; j < cnt * ns; ++j) r->sample_off[lo * ns + j + 1] = seg0 + soff[j + 1];
        for (uint64_t q = lo; q < hi; ++q)
            r->stats.matrix_bytes += 4 * msv_host::spl_matrix_words(S, poff[q + 1] - poff[q]);
        if (r->kept)
            for (uint64_t q = lo; q < hi; ++q) {
                const uint64_t Le = poff[q + 1] - poff[q];
                r->fm[q].assign(Le * M, 0.0f);
                r->fi[q].assign(Le * M, 0.0f);
                r->fd[q].assign(Le * M, 0.0f);
                r->rec[q].assign((Le + 1) * 6, 0u);
                if (!std::isfinite(r->env[q])) continue;
                const uint32_t* rec = host_ws.data() + base[q];
                const float* mat = reinterpret_cast<const float*>(rec + msv_host::spl_record_words(Le));
                std::copy(rec, rec + (Le + 1) * 6, r->rec[q].begin());
                for (uint64_t i = 0; i < Le; ++i) {
                    const float* row = mat + i * 3 * S * 64;
                    for (uint32_t k = 1; k <= K; ++k) {
                        const uint64_t l = (k - 1) / S, sl = (k - 1) % S;
                        r->fm[q][i * M + k] = row[sl * 64 + l];
                        r->fi[q][i * M + k] = row[(S + sl) * 64 + l];
                        r->fd[q][i * M + k] = row[(2 * S + sl) * 64 + l];
                    }
                }
            }
    }
    drain.disarm();
    s = stagedev::read_errors(p, kHostErrWord, st);
    if (s != MSV_OK && s != MSV_ERR_BAD_RESIDUE && s != MSV_ERR_SEQUENCE_TOO_LONG) return s;
    return give(s);
}

}  // namespace

extern "C" {

msv_status msv_spl_sample_batch(msv_dom_profile* p, const uint8_t* residues, const uint64_t* offsets, uint64_t n,
                                const msv_aln_item* items, uint64_t m, const msv_spl_options* options,
                                msv_spl_result** result) {
    msv_spl_options o;
    if (!read_sized(options, &o, sizeof(uint64_t))) return MSV_ERR_INVALID_ARGUMENT;
    return sample_batch(p, residues, offsets, n, items, m, o, result);
}

uint64_t msv_spl_result_count(const msv_spl_result* r) { return r ? r->env.size() : 0; }
uint64_t msv_spl_result_segments(const msv_spl_result* r) { return r ? r->segments.size() : 0; }

msv_status msv_spl_result_copy(const msv_spl_result* r, float* envelope_scores, uint64_t* sample_offsets,
                               msv_spl_segment* segments) {
    if (!r) return MSV_ERR_INVALID_ARGUMENT;
    if (envelope_scores) std::copy(r->env.begin(), r->env.end(), envelope_scores);
    if (sample_offsets) std::copy(r->sample_off.begin(), r->sample_off.end(), sample_offsets);
    if (segments) std::copy(r->segments.begin(), r->segments.end(), segments);
    return MSV_OK;
}

msv_status msv_spl_result_matrix(const msv_spl_result* r, uint64_t q, float* fM, float* fI, float* fD,
                                 uint32_t* records) {
    if (!r || !r->kept || q >= r->fm.size()) return MSV_ERR_INVALID_ARGUMENT;
    if (fM) std::copy(r->fm[q].begin(), r->fm[q].end(), fM);
    if (fI) std::copy(r->fi[q].begin(), r->fi[q].end(), fI);
    if (fD) std::copy(r->fd[q].begin(), r->fd[q].end(), fD);
    if (records) std::copy(r->rec[q].begin(), r->rec[q].end(), records);
    return MSV_OK;
}

msv_status msv_spl_result_stats(const msv_spl_result* r, msv_spl_stats* out) {
    if (!r || !out || out->struct_size < sizeof(uint32_t)) return MSV_ERR_INVALID_ARGUMENT;
    write_sized(out, r->stats);
    return MSV_OK;
}

void msv_spl_result_free(msv_spl_result* r) { delete r; }

msv_status msv_spl_describe(const msv_dom_profile* p, msv_spl_info* out) {
    if (!p || !out || out->struct_size < sizeof(uint32_t)) return MSV_ERR_INVALID_ARGUMENT;
    const splk::SplVariant* v = stagedev::find_by_shape(splk::spl_variants, p->v->S, p->v->isc);
    if (!v) return MSV_ERR_UNSUPPORTED_MODEL;
    DeviceGuard g(p->device);
    if (!g.ok) return MSV_ERR_NO_DEVICE;
    msv_spl_info info;
    std::memset(&info, 0, sizeof(info));
    info.states_per_lane = static_cast<uint32_t>(v->S);
    info.forward_blocks = msvrt::full_grid(p->device, v->fwd_fn, v->waves * 64);
    info.default_workspace_bytes = kDefaultWorkspace;
    std::snprintf(info.variant, sizeof(info.variant), "%s", v->name);
    msvrt::kernel_footprint(v->fwd_fn, &info.forward_scratch_bytes, &info.forward_lds_bytes);
    msvrt::kernel_footprint(splk::sample_fn(), &info.sample_scratch_bytes, &info.sample_lds_bytes);
    write_sized(out, info);
    return MSV_OK;
}

}  // extern "C"
