// spl_device.cpp -- C-ABI of the split stage (msv.h) on the HIP runtime.
//
// The stage runs on a msv_dom_profile as the alignment stage does (aln_device.cpp): the recording kernel of
// spl_kernel.hip reads the tables the domain stage's variant installed, the sampler a flat table of the float32
// transition odds made per call.  The host packs the items' residues into a CSR batch of their own (item q is
// sequence q of it), cuts the items into chunks that fit the workspace as the Viterbi trace's are cut, and runs three
// launches per chunk: the recording Forward on a launch slot of its own, the sampler's count pass and, after a host
// scan, its place pass.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>
#include <vector>

#include "dom_profile.h"
#include "hip_rt.h"
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

constexpr uint64_t kDefaultWorkspace = 1ull << 30;
constexpr uint32_t kDefaultSamples = 200;
constexpr uint64_t kDefaultSeed = 42;

const splk::SplVariant* variant_of(const msv_dom_profile* p) {
    int n = 0;
    const splk::SplVariant* all = splk::spl_variants(&n);
    for (int i = 0; i < n; ++i)
        if (all[i].S == p->v->S && all[i].isc == p->v->isc) return &all[i];
    return nullptr;
}

uint32_t full_grid(int device, const void* fn, int waves) {
    int blocks = 0;
    (void)msvrt::resident_blocks(device, fn, waves * 64, &blocks);
    return static_cast<uint32_t>(std::max(1, blocks));
}

float elapsed(const msvrt::Event& a, const msvrt::Event& b) {
    float ms = 0.0f;
    return hipEventElapsedTime(&ms, a, b) == hipSuccess ? ms : 0.0f;
}

template <class T>
hipError_t upload(DeviceBuffer<T>& d, const std::vector<T>& h, hipStream_t st) {
    hipError_t e = d.reserve(h.size());
    if (e == hipSuccess && !h.empty())
        e = hipMemcpyAsync(d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, st);
    return e;
}

msv_status sample_batch(msv_dom_profile* p, const uint8_t* residues, const uint64_t* offsets, uint64_t n,
                        const msv_aln_item* items, uint64_t m, const msv_spl_options& opt, msv_spl_result** result) {
    if (!p || !result || (n && !offsets) || (m && !items)) return MSV_ERR_INVALID_ARGUMENT;
    *result = nullptr;
    if (n >= (1ull << 32) || m >= (1ull << 32)) return MSV_ERR_INVALID_ARGUMENT;
    const uint32_t ns = opt.n_samples ? opt.n_samples : kDefaultSamples;
    const uint64_t seed = opt.seed_set ? opt.seed : kDefaultSeed;
    if (ns >= (1u << 24) || m * ns >= (1ull << 32)) return MSV_ERR_INVALID_ARGUMENT;
    uint64_t longest = 0, total = 0;
    msv_status s = n ? msvrt::csr_extent(offsets, n, &longest, &total) : MSV_OK;
    if (s != MSV_OK) return s;
    if (total && !residues) return MSV_ERR_INVALID_ARGUMENT;
    if (longest >= (1ull << 31)) return MSV_ERR_SEQUENCE_TOO_LONG;
    for (uint64_t q = 0; q < m; ++q) {
        const msv_aln_item& it = items[q];
        if (it.seq >= n || it.i_from < 1 || it.i_from > it.i_to || it.i_to > offsets[it.seq + 1] - offsets[it.seq])
            return MSV_ERR_INVALID_ARGUMENT;
    }
    const splk::SplVariant* v = variant_of(p);
    if (!v) return MSV_ERR_UNSUPPORTED_MODEL;
    const uint64_t S = static_cast<uint64_t>(v->S);
    const uint32_t M = p->model_length, K = M - 1;

    auto* r = new (std::nothrow) msv_spl_result;
    if (!r) return MSV_ERR_OUT_OF_MEMORY;
    struct Guard {
        msv_spl_result* r;
        ~Guard() { delete r; }
    } guard{r};
    r->M = M;
    r->kept = opt.keep_matrix != 0;
    r->stats.n_samples = ns;
    r->stats.seed = seed;
    r->env.assign(m, std::nanf(""));
    r->sample_off.assign(m * ns + 1, 0);
    if (r->kept) r->fm.resize(m), r->fi.resize(m), r->fd.resize(m), r->rec.resize(m);
    auto give = [&](msv_status st) {
        *result = r;
        guard.r = nullptr;
        return st;
    };
    if (m == 0) return give(MSV_OK);

    // the items as a batch of their own, and the chunks, before anything is launched
    const uint64_t budget = opt.workspace_bytes ? opt.workspace_bytes : kDefaultWorkspace;
    std::vector<uint64_t> poff(m + 1, 0), bytes(m), cuts(m + 1, 0), base(m);
    std::vector<uint32_t> lc(m), sel(m);
    for (uint64_t q = 0; q < m; ++q) {
        const uint64_t Le = items[q].i_to - items[q].i_from + 1;
        poff[q + 1] = poff[q] + Le;
        bytes[q] = msv_host::spl_item_bytes(S, Le);
        lc[q] = static_cast<uint32_t>(offsets[items[q].seq + 1] - offsets[items[q].seq]);
        sel[q] = static_cast<uint32_t>(q);
    }
    uint64_t n_chunks = 0;
    s = msv_vit_trace_chunk_cuts(bytes.data(), m, budget, cuts.data(), &n_chunks);
    if (s == MSV_ERR_OUT_OF_MEMORY) return give(s);  // (nothing launched: the result says so, chunks = 0)
    if (s != MSV_OK) return s;
    std::vector<uint8_t> packed(poff[m]);
    for (uint64_t q = 0; q < m; ++q)
        std::copy_n(residues + offsets[items[q].seq] + items[q].i_from - 1, poff[q + 1] - poff[q],
                    packed.begin() + static_cast<std::ptrdiff_t>(poff[q]));
    uint64_t chunk_words = 0, chunk_items = 0;
    std::vector<uint32_t> counts(n_chunks);
    for (uint64_t c = 0; c < n_chunks; ++c) {
        uint64_t at = 0;
        for (uint64_t q = cuts[c]; q < cuts[c + 1]; ++q) {
            base[q] = at;
            at += bytes[q] / 4;
        }
        chunk_words = std::max(chunk_words, at);
        counts[c] = static_cast<uint32_t>(cuts[c + 1] - cuts[c]);
        chunk_items = std::max<uint64_t>(chunk_items, counts[c]);
    }

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
    MSV_HIP(d_ws.reserve(chunk_words));
    MSV_HIP(d_scounts.reserve(chunk_items * ns));
    msvrt::StreamDrain drain(st);
    MSV_HIP(sg.upload(packed.data(), poff.data(), 0, m, true, st, st));
    MSV_HIP(upload(d_lc, lc, st));
    MSV_HIP(upload(d_sel, sel, st));
    MSV_HIP(upload(d_counts, counts, st));
    MSV_HIP(upload(d_base, base, st));
    MSV_HIP(upload(d_tr, tr, st));
    MSV_HIP(d_items.reserve(m));
    MSV_HIP(hipMemcpyAsync(d_items, items, m * sizeof(msv_aln_item), hipMemcpyHostToDevice, st));
    // an item the kernel refuses keeps what is set here: a NaN score
    MSV_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(sg.d_scores.get()), 0x7fc00000, m, st));

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
        {
            const uint64_t need = (cnt + static_cast<uint64_t>(v->waves) - 1) / static_cast<uint64_t>(v->waves);
            const uint32_t blocks =
                static_cast<uint32_t>(std::min<uint64_t>(full_grid(p->device, v->fwd_fn, v->waves), need));
            MSV_HIP(p->kernels.run(st, stagedev::lazy(p, st), p->d_words.get(), 2, [&](uint32_t* counter) {
                a.counter = counter;
                return splk::spl_launch(v->fwd_fn, v->waves, blocks, a, st);
            }));
        }
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
    std::memset(&o, 0, sizeof(o));
    if (options) {
        if (options->struct_size < sizeof(uint64_t)) return MSV_ERR_INVALID_ARGUMENT;
        std::memcpy(&o, options, static_cast<size_t>(std::min<uint64_t>(options->struct_size, sizeof(o))));
    }
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
    msv_spl_stats st = r->stats;
    const uint32_t size = std::min<uint32_t>(out->struct_size, static_cast<uint32_t>(sizeof(st)));
    st.struct_size = size;
    std::memcpy(out, &st, size);
    return MSV_OK;
}

void msv_spl_result_free(msv_spl_result* r) { delete r; }

msv_status msv_spl_describe(const msv_dom_profile* p, msv_spl_info* out) {
    if (!p || !out || out->struct_size < sizeof(uint32_t)) return MSV_ERR_INVALID_ARGUMENT;
    const splk::SplVariant* v = variant_of(p);
    if (!v) return MSV_ERR_UNSUPPORTED_MODEL;
    DeviceGuard g(p->device);
    if (!g.ok) return MSV_ERR_NO_DEVICE;
    msv_spl_info info;
    std::memset(&info, 0, sizeof(info));
    info.states_per_lane = static_cast<uint32_t>(v->S);
    info.forward_blocks = full_grid(p->device, v->fwd_fn, v->waves);
    info.default_workspace_bytes = kDefaultWorkspace;
    std::snprintf(info.variant, sizeof(info.variant), "%s", v->name);
    hipFuncAttributes fa{};
    if (hipFuncGetAttributes(&fa, v->fwd_fn) == hipSuccess) {
        info.forward_scratch_bytes = static_cast<uint32_t>(fa.localSizeBytes);
        info.forward_lds_bytes = static_cast<uint32_t>(fa.sharedSizeBytes);
    }
    if (hipFuncGetAttributes(&fa, splk::sample_fn()) == hipSuccess) {
        info.sample_scratch_bytes = static_cast<uint32_t>(fa.localSizeBytes);
        info.sample_lds_bytes = static_cast<uint32_t>(fa.sharedSizeBytes);
    }
    const uint32_t size = std::min<uint32_t>(out->struct_size, static_cast<uint32_t>(sizeof(info)));
    info.struct_size = size;
    std::memcpy(out, &info, size);
    return MSV_OK;
}

}  // extern "C"
