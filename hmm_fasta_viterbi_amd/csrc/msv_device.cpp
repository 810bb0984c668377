// msv_device.cpp -- C-ABI of the device hot path (msv.h) on the HIP runtime.
//
// Replaces the per-call OpenCL orchestration of MSV_HMM::parallel_run_on_sequence
// (algorithms/MSV_HMM.cpp:269-430: a context, 23 buffers, a JIT program build and 9-14 kernel
// launches per residue, for every sequence) with: one device-resident profile built once
// (kernel-layout emission table + per-length transition table), and one persistent kernel
// launch per batch.  Status codes are returned, never printed-and-continued (:198-203).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <thread>
#include <vector>

#include "hip_rt.h"
#include "host_cpu.h"
#include "launch_ring.h"
#include "msv.h"
#include "msv_kernel.h"
#include "msv_plan.h"

using msvplan::CallPlan;
using msvplan::kLaunchSlots;
using msvrt::csr_extent;
using msvrt::CsrStaging;
using msvrt::DeviceBuffer;
using msvrt::DeviceGuard;
using msvrt::hip_status;
using msvrt::kChunkBytes;
using msvrt::kMaxLaunchSeqs;
using msvrt::mapped_host;
using msvrt::PinnedBuffer;
using msvrt::StreamDrain;

// table_layout.cpp builds the tables without msv_kernel.h
static_assert(msvk::kAminoAcids == 20 && msvk::kPoisonRow == 20 && msvk::kTableRows == 21, "table_layout.cpp's rows");
static_assert(msvplan::kGridMaxProfiles == msvk::kGridMaxProfiles, "msv_plan.h's fused launch");

namespace {

constexpr uint32_t kDefaultMaxLength = 131072;
constexpr uint32_t kOrderBins = 4096;  // lengths >= 4095 share the longest bin
// Every launch of one profile takes the next of kLaunchSlots (msv_plan.h) device counter pairs {next index, waves
// left} (and, for the longest-first order, the next histogram), so launches on different streams
// never share a counter; a slot is reused only after its previous launch (an event wait when the
// streams differ).  d_words: [2k, 2k+1] = slot k's counters, [kErrWord] = sticky error bits,
// [kErrWord + 1 + a] = the error bits of asynchronous staging slot a (msv_score_batch_async),
// [kHostErrWord] = the error bits of synchronous host calls (msv_score_batch), which report and clear only
// their own: bits latched by msv_score_batch_device launches stay for msv_profile_check.
constexpr int kAsyncSlots = 3;
constexpr int kErrWord = 2 * kLaunchSlots;
constexpr int kHostErrWord = kErrWord + 1 + kAsyncSlots;
constexpr int kWords = kHostErrWord + 1;

// MSV_HMM::init_transitions_depend_on_seq (MSV_HMM.cpp:59-64) for every length < n, with the
// host's logf (never a device logf, so the per-sequence constants are the reference's bits).
// Returns a copy of the first n entries: the shared cache may grow under another thread (one host
// thread per device in msv_score_batch_multi), so nothing refers into it outside the lock.
std::vector<float2> host_length_table(uint32_t n) {
    static std::mutex mu;
    static std::vector<float2> table;
    std::lock_guard<std::mutex> lock(mu);
    if (table.size() < n) {
        const size_t old = table.size();
        table.resize(n);
        for (size_t L = old; L < n; ++L) {
            float loop, move;
            msv_sequence_transitions(L, &loop, &move);
            table[L] = make_float2(loop, move);
        }
    }
    return std::vector<float2>(table.begin(), table.begin() + n);
}

// Launch slots of one profile (see kLaunchSlots and launch_ring.h).
using LaunchRing = msvrt::LaunchRing<kLaunchSlots>;

// The shapes of msvk::variants() and msvk::coop_variants(), index for index, for the policy (msv_plan.h).
const msvplan::Tables& plan_tables() {
    static const msvplan::Tables tables = [] {
        msvplan::Tables t;
        int count = 0;
        const msvk::Variant* all = msvk::variants(&count);
        for (int i = 0; i < count; ++i) {
            const msvk::Variant& v = all[i];
            t.variants.push_back({v.G, v.S, v.waves, v.pf, v.streams, v.sa, v.big, v.grid_fn != nullptr});
        }
        const msvk::CoopVariant* coop = msvk::coop_variants(&count);
        for (int i = 0; i < count; ++i)
            t.coop.push_back({coop[i].waves, coop[i].S, coop[i].halo, coop[i].sa, coop[i].grid_fn != nullptr});
        return t;
    }();
    return tables;
}

}  // namespace

// One kernel instantiation with its emission table (in that variant's layout) and grid.
struct Plan {
    const msvk::Variant* v = nullptr;
    const msvk::CoopVariant* cv = nullptr;  // the cooperative plan (msv_coop.hip) instead of a variant
    DeviceBuffer<float4> d_etab;
    int blocks = 0;  // persistent grid size
    int groups_per_block = 0;
};

struct msv_profile {
    int device = 0;
    uint32_t model_length = 0;  // LENG + 1
    Plan main;                    // throughput plan (every launch unless the batch is small)
    Plan lat;                     // latency plan for small batches (G = 64), may equal main's variant
    Plan mid;                     // mid-size batches (G = 32), large G = 16 profiles only
    Plan fused;                   // the table in another profile's latency layout (fused grid launches)
    Plan coop;                    // one sequence per workgroup, the row over its waves (msv_coop.hip)
    Plan coop_fused;              // the table in another profile's cooperative layout (fused grid launches)
    msvplan::PlanSet chosen;      // which of them exist, and up to how many sequences each is taken (msv_plan.h)
    bool force = false;           // msv_profile_set_variant: main plan for every batch size
    float tr_B_Mk = 0, tr_E_C = 0, tr_E_J = 0;
    std::vector<float> emission_scores;  // host copy [20][model_length] (for re-layout)
    DeviceBuffer<float2> d_lentab;
    uint32_t lentab_n = 0;
    DeviceBuffer<uint32_t> d_words;  // kLaunchSlots x {dequeue counter, waves still running}, sticky error bits
    DeviceBuffer<uint32_t> d_hist;  // kLaunchSlots longest-first counting-sort scratches [hist | cursors]
    DeviceBuffer<uint8_t> d_dummy;  // device API: a readable residue byte for launches given no residues
    LaunchRing kernels, orders;   // launch slots of the MSV kernel and of the order sort
    msvrt::Stream stream;
    hipStream_t bound = nullptr;  // msv_profile_bind_stream: a caller stream guaranteed alive while bound
    // host-API pipeline (msv_score_batch): a second compute stream, a copy stream and piece events
    msvrt::Stream stream2, copy_stream;
    msvrt::Stream offsets_stream;  // msv_score_batch_async: the offsets' H2D, beside the residues'
    std::vector<msvrt::Event> events;
    // host-API staging (msv_score_batch, msv_score_grid; msv_score_fasta_device's order and scores)
    CsrStaging host;
    PinnedBuffer<float> h_sc;  // pinned score staging of small calls with pageable destinations
    uint32_t pipe_first_den = 4, pipe_growth = 2;  // piece sizes: total / first_den, then x growth
    uint32_t pipe_streams = 2;                      // compute streams the pieces alternate over
    bool zero_copy = true;  // page-locked residues read in place (msv_debug_set_zero_copy turns it off)
    bool zc_wide = true;    // ... by the wide-block twins of residue-block variants (msv_debug_set_zero_copy 2: off)
    // msv_score_batch_async: kAsyncSlots staging sets, so the H2D of one call runs under the kernel
    // of the call before it
    struct AsyncSlot {
        CsrStaging staged;
        PinnedBuffer<uint32_t> h_err;  // pinned copy of the slot's error word
        const float* direct = nullptr;  // page-locked destination written by the kernel (errors: scan)
        uint64_t n = 0;
        msvrt::Event copied, done, off_copied;
        uint64_t ticket = 0;
        bool pending = false;
    } async[kAsyncSlots];
    uint64_t next_ticket = 1;
    uint64_t* d_stamps = nullptr;  // diagnostic timeline buffer (tools only), or nullptr
    bool stamp_clock = false;      // d_stamps is for the CLOCK twins (kStampWords per wave: bench.py clock_GHz)
    hipEvent_t time_start = nullptr, time_stop = nullptr;  // msv_debug_time_next_launch (one launch)
    msvrt::Event done;             // grid API: joins this profile's stream back to the caller's
    hipStream_t shared = nullptr;  // shared_stream(device) once a host grid call used it
};


// One stream per device that the library never destroys: host grid calls launch on it, so every
// profile of the grid may leave its slot event unrecorded (a per-profile event record is a packet on
// the stream: 24 of them put ~115 us between a fused grid launch and its scores' D2H).
static hipStream_t shared_stream(int device) {
    static std::mutex mu;
    static std::map<int, hipStream_t> streams;
    std::lock_guard<std::mutex> lock(mu);
    auto it = streams.find(device);
    if (it != streams.end()) return it->second;
    hipStream_t st = nullptr;
    if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) return nullptr;
    streams[device] = st;
    return st;
}

// Streams on which a launch may leave its slot event unrecorded (LaunchRing): they stay alive
// until the profile is destroyed or the binding ends (msv_profile_bind_stream flushes first), or
// forever (shared_stream).
static bool lazy_stream(const msv_profile* p, hipStream_t st) {
    return st == p->stream || st == p->stream2 || (p->bound && st == p->bound) || (p->shared && st == p->shared);
}

// The status of a kernel's latched error bits (msv_kernel.h kErr*), most specific first.
static msv_status err_status(uint32_t err) {
    if (err & msvk::kErrBadOrder) return MSV_ERR_INVALID_ARGUMENT;  // an order entry outside the batch
    if (err & msvk::kErrBadResidue) return MSV_ERR_BAD_RESIDUE;
    if (err & msvk::kErrTooLong) return MSV_ERR_SEQUENCE_TOO_LONG;
    return MSV_OK;
}

// Whether a batch whose scores went straight to host memory had an error: a bad residue leaves +inf,
// a too-long sequence or a bad order entry NaN (msv_kernel.hip); valid scores are finite or -inf.  The
// classification of a positive answer comes from the kernel's error bits (err_status), since a NaN can
// also come out of a bad residue's +inf meeting a -inf.
static msv_status scan_scores(const float* scores, uint64_t n) {
    bool inf = false, nan = false;
    for (uint64_t i = 0; i < n; ++i) {
        const float x = scores[i];
        inf |= x == std::numeric_limits<float>::infinity();
        nan |= x != x;
    }
    if (inf) return MSV_ERR_BAD_RESIDUE;
    if (nan) return MSV_ERR_SEQUENCE_TOO_LONG;
    return MSV_OK;
}

// The persistent grid of `kernel` on the device; one block per CU when the occupancy query fails.
static msv_status grid_blocks(int device, const void* kernel, int waves, int* blocks) {
    const hipError_t e = msvrt::resident_blocks(device, kernel, waves * 64, blocks);
    return *blocks > 0 ? MSV_OK : hip_status(e);
}

// Lays the MSV table out for variant v (msv_host::msv_variant_table), uploads it and sizes the grid.
static msv_status install_plan(msv_profile* p, const msvk::Variant* v, Plan& plan) {
    std::vector<float> tab =
        msv_host::msv_variant_table(p->emission_scores.data(), p->model_length, v->G, v->S, v->sa);
    if (msvk::lazy_e_rows(v->S, v->waves, v->pf, v->big, v->sa, v->streams)) {  // the kernel stages the bound table behind the rows
        const std::vector<float> emax =
            msv_host::msv_lazy_bound_table(p->emission_scores.data(), p->model_length, v->G, v->S);
        tab.insert(tab.end(), emax.begin(), emax.end());
    }
    // (the old table may be read by an in-flight launch on any stream the caller used: replace_with)
    MSV_HIP(plan.d_etab.replace_with(reinterpret_cast<const float4*>(tab.data()), tab.size() / 4));
    plan.v = v;
    plan.groups_per_block = v->waves * (64 / v->G) * v->streams;
    return grid_blocks(p->device, v->fn, v->waves, &plan.blocks);
}

static void drop_plan(Plan& plan) {
    if (plan.d_etab) (void)hipDeviceSynchronize();  // may be read by an in-flight launch
    plan = Plan{};
}

// Lays p's table out for cooperative variant cv (msv_host::msv_coop_table) into `plan` (d_etab, cv).
static msv_status install_coop_table(msv_profile* p, const msvk::CoopVariant* cv, Plan& plan) {
    const std::vector<float> tab =
        msv_host::msv_coop_table(p->emission_scores.data(), p->model_length, cv->waves, cv->S, cv->sa, cv->halo);
    MSV_HIP(plan.d_etab.replace_with(reinterpret_cast<const float4*>(tab.data()), tab.size() / 4));
    plan.v = nullptr;
    plan.cv = cv;
    plan.blocks = 0;
    plan.groups_per_block = 1;
    return MSV_OK;
}

// Chooses the profile's plans (msv_plan.h choose; `forced`: the index of the variant msv_profile_set_variant
// named, or -1) and installs them: every chosen plan's table laid out and uploaded and its grid sized, every
// other plan dropped.
static msv_status install_plans(msv_profile* p, int forced) {
    int cus = 0, count = 0;
    MSV_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, p->device));
    const msvk::Variant* all = msvk::variants(&count);
    const msvk::CoopVariant* coop = msvk::coop_variants(&count);
    const auto blocks_of = [&](msvplan::Kind kind, int i) {
        int blocks = 0;
        if (kind == msvplan::kCoop) (void)grid_blocks(p->device, coop[i].fn, coop[i].waves, &blocks);
        else (void)grid_blocks(p->device, all[i].fn, all[i].waves, &blocks);
        return blocks;
    };
    const bool same_EJ = std::memcmp(&p->tr_E_C, &p->tr_E_J, sizeof(float)) == 0;
    const msvplan::PlanSet ps = msvplan::choose(plan_tables(), p->model_length - 1, same_EJ, forced, cus, blocks_of);
    if (ps.main < 0) return MSV_ERR_UNSUPPORTED_MODEL;
    p->force = forced >= 0;  // a forced variant runs every batch (tests, tools/tune.py)
    p->chosen = msvplan::PlanSet{};  // (a failure below leaves every batch on the main plan)
    const struct {
        int index;
        Plan& plan;
    } plans[] = {{ps.main, p->main}, {ps.lat, p->lat}, {ps.mid, p->mid}};
    for (const auto& x : plans) {
        if (x.index < 0) {
            drop_plan(x.plan);
            continue;
        }
        const msv_status s = install_plan(p, &all[x.index], x.plan);
        if (s != MSV_OK) return s;
    }
    if (ps.coop < 0) {
        drop_plan(p->coop);
    } else {
        msv_status s = install_coop_table(p, &coop[ps.coop], p->coop);
        if (s == MSV_OK) s = grid_blocks(p->device, coop[ps.coop].fn, coop[ps.coop].waves, &p->coop.blocks);
        if (s != MSV_OK) return s;
    }
    p->chosen = ps;
    return MSV_OK;
}

extern "C" {

msv_status msv_device_count(int* count) {
    if (!count) return MSV_ERR_INVALID_ARGUMENT;
    *count = 0;
    hipError_t e = hipGetDeviceCount(count);
    if (e != hipSuccess) {
        *count = 0;
        return MSV_ERR_NO_DEVICE;
    }
    return MSV_OK;
}

void msv_profile_destroy(msv_profile* p) {
    if (!p) return;
    DeviceGuard g(p->device);
    // work still queued on any stream (an unwaited msv_score_batch_async call, a device call on the
    // caller's stream) may use the buffers and pinned staging that the members' destructors free
    (void)hipDeviceSynchronize();
    delete p;
}

msv_status msv_profile_reserve_length(msv_profile* p, uint64_t max_length) {
    if (!p) return MSV_ERR_INVALID_ARGUMENT;
    if (max_length >= (1ull << 31)) return MSV_ERR_SEQUENCE_TOO_LONG;
    const uint32_t need = static_cast<uint32_t>(max_length) + 1;
    if (need <= p->lentab_n) return MSV_OK;
    DeviceGuard g(p->device);
    if (!g.ok) return MSV_ERR_NO_DEVICE;
    const uint32_t n = std::max(need, p->lentab_n * 2);
    const std::vector<float2> host = host_length_table(n);
    // (the old table may still be read by an in-flight launch on any stream the caller used: replace_with)
    MSV_HIP(p->d_lentab.replace_with(host.data(), n));
    p->lentab_n = n;
    return MSV_OK;
}

msv_status msv_profile_create(int device, const float* emission_scores, uint32_t model_length, float tr_B_Mk,
                              float tr_E_C, float tr_E_J, msv_profile** out) {
    if (!emission_scores || !out || model_length < 2) return MSV_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return MSV_ERR_NO_DEVICE;
    if (device < 0 || device >= ndev) return MSV_ERR_NO_DEVICE;
    DeviceGuard g(device);
    if (!g.ok) return MSV_ERR_NO_DEVICE;
    struct Destroy {
        void operator()(msv_profile* p) const { msv_profile_destroy(p); }
    };
    std::unique_ptr<msv_profile, Destroy> p(new (std::nothrow) msv_profile);  // destroyed on every error return
    if (!p) return MSV_ERR_OUT_OF_MEMORY;
    p->device = device;
    p->model_length = model_length;
    p->tr_B_Mk = tr_B_Mk;
    p->tr_E_C = tr_E_C;
    p->tr_E_J = tr_E_J;
    p->emission_scores.assign(emission_scores, emission_scores + static_cast<size_t>(20) * model_length);
    MSV_HIP(p->stream.create(hipStreamNonBlocking));
    // every launch slot's event up front: created lazily, the first kLaunchSlots launches of a fresh
    // profile each paid an event creation (~10 us; 24 of them in one fused grid call)
    MSV_HIP(p->kernels.create_events());
    MSV_HIP(p->orders.create_events());
    MSV_HIP(p->d_words.reserve(kWords));
    MSV_HIP(hipMemset(p->d_words, 0, kWords * sizeof(uint32_t)));
    MSV_HIP(p->d_dummy.reserve(64));
    MSV_HIP(hipMemset(p->d_dummy, 0, 64));
    msv_status s = install_plans(p.get(), -1);  // (MSV_ERR_UNSUPPORTED_MODEL: no variant covers the model)
    if (s == MSV_OK) s = msv_profile_reserve_length(p.get(), kDefaultMaxLength - 1);
    if (s != MSV_OK) return s;
    *out = p.release();
    return MSV_OK;
}

int msv_variant_count(void) {
    int count = 0;
    (void)msvk::variants(&count);
    return count;
}

const char* msv_variant_name(int i) {
    int count = 0;
    const msvk::Variant* all = msvk::variants(&count);
    return (i >= 0 && i < count) ? all[i].name : nullptr;
}

msv_status msv_profile_set_variant(msv_profile* p, const char* name) {
    if (!p || !name) return MSV_ERR_INVALID_ARGUMENT;
    int count = 0;
    const msvk::Variant* all = msvk::variants(&count);
    for (int i = 0; i < count; ++i) {
        if (std::strcmp(all[i].name, name) != 0) continue;
        if (static_cast<uint32_t>(all[i].G * all[i].S) < p->model_length - 1) return MSV_ERR_UNSUPPORTED_MODEL;
        DeviceGuard g(p->device);
        if (!g.ok) return MSV_ERR_NO_DEVICE;
        return install_plans(p, i);
    }
    return MSV_ERR_INVALID_ARGUMENT;
}

// Diagnostics, deliberately not in msv.h: a device buffer of msvk::kStampWords (6) uint64 per wave of the
// persistent grid that receives {start, end (s_memrealtime, 100 MHz), rows issued, xcc<<32|block, shader
// clock start, end (s_memtime)} for every wave of subsequent launches (tools/wave_timeline.py, bench.py's
// clock_GHz).  nullptr switches it off.
msv_status msv_debug_set_stamps(msv_profile* p, uint64_t* d_stamps) {
    if (!p) return MSV_ERR_INVALID_ARGUMENT;
    p->d_stamps = d_stamps;
    p->stamp_clock = false;
    return MSV_OK;
}

// Diagnostics (bench.py roofline.clock_GHz), not in msv.h: subsequent launches of plans that have a CLOCK twin
// (msv_kernel_impl.h clock_fn) run it and write msvk::kStampWords (6) uint64 per wave -- the 4 stamps above plus
// shader-clock ticks (s_memtime) at the wave's start and end; launches of other plans write nothing.
// nullptr switches it off.
msv_status msv_debug_set_clock_stamps(msv_profile* p, uint64_t* d_stamps) {
    if (!p) return MSV_ERR_INVALID_ARGUMENT;
    p->d_stamps = d_stamps;
    p->stamp_clock = d_stamps != nullptr;
    return MSV_OK;
}

// Diagnostics (not in msv.h): the host pipeline's piece plan -- the first piece is 1/first_den of the
// batch, each next one `growth` times larger; first_den = 0 scores the batch as one piece; pieces
// alternate over `streams` (1 or 2) compute streams.
msv_status msv_debug_set_pipeline(msv_profile* p, uint32_t first_den, uint32_t growth, uint32_t streams) {
    if (!p || growth == 0 || streams < 1 || streams > 2) return MSV_ERR_INVALID_ARGUMENT;
    p->pipe_first_den = first_den;
    p->pipe_growth = growth;
    p->pipe_streams = streams;
    return MSV_OK;
}

// Diagnostics (not in msv.h): the profile's next MSV launch updates `start` / `stop` (hipEvent_t, created
// with timing) with its own start and end through hipExtLaunchKernel -- the kernel duration without the
// two marker packets (~4 us each on the stream) that event records around the launch would add.
msv_status msv_debug_time_next_launch(msv_profile* p, void* start, void* stop) {
    if (!p) return MSV_ERR_INVALID_ARGUMENT;
    p->time_start = static_cast<hipEvent_t>(start);
    p->time_stop = static_cast<hipEvent_t>(stop);
    return MSV_OK;
}

// Diagnostics (not in msv.h): batches up to n sequences take the cooperative plan (tools/coop_sweep.py;
// 0 turns it off).  Returns MSV_ERR_UNSUPPORTED_MODEL when the profile has no cooperative plan.
msv_status msv_debug_set_coop_max_n(msv_profile* p, uint64_t n) {
    if (!p) return MSV_ERR_INVALID_ARGUMENT;
    if (!p->coop.cv) return MSV_ERR_UNSUPPORTED_MODEL;
    p->chosen.coop_max_n = n;
    return MSV_OK;
}

// Diagnostics (not in msv.h): how msv_score_batch treats page-locked residues.  on: 0 = copied (pipeline),
// 1 = read in place, 2 = read in place but without the wide-block twins (A/B of the 64-byte superblock
// requests against the 16-byte block requests).
msv_status msv_debug_set_zero_copy(msv_profile* p, int on) {
    if (!p || on < 0 || on > 2) return MSV_ERR_INVALID_ARGUMENT;
    p->zero_copy = on != 0;
    p->zc_wide = on != 2;
    return MSV_OK;
}

int msv_debug_grid_waves(const msv_profile* p) {
    if (!p) return 0;
    const int lat = p->lat.v ? p->lat.blocks * p->lat.v->waves : 0;
    const int mid = p->mid.v ? p->mid.blocks * p->mid.v->waves : 0;
    return std::max({p->main.blocks * p->main.v->waves, lat, mid});  // the stamps buffer must fit every plan
}

msv_status msv_profile_create_from_hmm(int device, const msv_hmm* hmm, msv_profile** out) {
    if (!hmm || !out) return MSV_ERR_INVALID_ARGUMENT;
    const size_t M = msv_hmm_model_length(hmm);
    std::vector<float> es(M * 20);
    float b, c, j;
    msv_status s = msv_hmm_msv_scores(hmm, es.data(), &b, &c, &j);
    if (s != MSV_OK) return s;
    return msv_profile_create(device, es.data(), static_cast<uint32_t>(M), b, c, j, out);
}

msv_status msv_profile_describe(const msv_profile* p, msv_kernel_info* out) {
    if (!p || !out) return MSV_ERR_INVALID_ARGUMENT;
    std::memset(out, 0, sizeof(*out));
    out->model_length = p->model_length;
    const msvk::Variant* v = p->main.v;
    out->lanes_per_group = static_cast<uint32_t>(v->G);
    out->states_per_lane = static_cast<uint32_t>(v->S);
    out->waves_per_block = static_cast<uint32_t>(v->waves);
    out->lds_rows = static_cast<uint32_t>(v->lds_rows);
    out->lds_bytes = static_cast<uint32_t>(v->lds_rows * v->G * (v->sa ? v->sa : v->S) * 4);
    out->blocks = static_cast<uint32_t>(p->main.blocks);
    out->max_length = p->lentab_n ? p->lentab_n - 1 : 0;
    out->device = p->device;
    std::snprintf(out->variant, sizeof(out->variant), "%s", v->name);
    // the small-batch (latency) plan, if this profile has one
    if (p->lat.v) {
        std::snprintf(out->latency_variant, sizeof(out->latency_variant), "%s", p->lat.v->name);
        out->latency_blocks = static_cast<uint32_t>(p->lat.blocks);
        out->latency_max_n = p->chosen.lat_max_n;
    }
    if (p->coop.cv) {
        std::snprintf(out->coop_variant, sizeof(out->coop_variant), "%s", p->coop.cv->name);
        out->coop_blocks = static_cast<uint32_t>(p->coop.blocks);
        out->coop_max_n = p->chosen.coop_max_n;
    }
    if (p->mid.v) {
        std::snprintf(out->mid_variant, sizeof(out->mid_variant), "%s", p->mid.v->name);
        out->mid_blocks = static_cast<uint32_t>(p->mid.blocks);
        out->mid_max_n = p->chosen.mid_max_n;
    }
    return MSV_OK;
}

// The plan a launch of n sequences takes (msv_plan.h which).
static const Plan& select_plan(const msv_profile* p, uint64_t n, bool latency_ok, bool host_residues = false) {
    switch (msvplan::which(p->chosen, n, latency_ok, host_residues)) {
        case msvplan::kCoop: return p->coop;
        case msvplan::kLatency: return p->lat;
        case msvplan::kMid: return p->mid;
        default: return p->main;
    }
}

static bool order_needless(const msv_profile* p, uint64_t n, bool host_residues) {
    return msvplan::order_needless(p->chosen, n, host_residues, p->coop.blocks);
}

const char* msv_profile_variant_for(const msv_profile* p, uint64_t n) {
    if (!p || !p->main.v) return "";
    const Plan& plan = select_plan(p, n, true);
    return plan.cv ? plan.cv->name : plan.v->name;
}

// The kernel arguments of one batch on `plan` of `p`: no stamps, the device launches' error word and (for the
// kernels that dequeue) counter slot 0 until the caller says otherwise.
static msvk::KernelArgs kernel_args(const msv_profile* p, const Plan& plan, const uint8_t* d_residues,
                                    uint64_t residues_len, const uint64_t* d_offsets, uint64_t n,
                                    const uint32_t* d_order, float* d_scores) {
    msvk::KernelArgs a{};
    a.etab = plan.d_etab;
    a.residues = residues_len ? d_residues : p->d_dummy;
    a.offsets = d_offsets;
    a.order = d_order;
    a.lentab = p->d_lentab;
    a.scores = d_scores;
    a.counter = p->d_words;
    a.errors = p->d_words + kErrWord;
    a.n = n;
    a.lentab_n = p->lentab_n;
    a.tr_B_Mk = p->tr_B_Mk;
    a.tr_E_C = p->tr_E_C;
    a.tr_E_J = p->tr_E_J;
    a.stamps = nullptr;
    return a;
}

// One MSV launch.  `latency_ok`: a batch of few sequences may take the latency plan (not for the
// pieces of a host pipeline, whose kernels must share the CUs with the next piece's).
static msv_status launch_batch(msv_profile* p, const uint8_t* d_residues, uint64_t residues_len,
                               const uint64_t* d_offsets, uint64_t n, const uint32_t* d_order, float* d_scores,
                               void* stream, bool latency_ok, uint32_t* d_errors = nullptr,
                               bool host_residues = false) {
    if (!p) return MSV_ERR_INVALID_ARGUMENT;
    if (n == 0) return MSV_OK;
    if (!d_offsets || !d_scores || (residues_len && !d_residues)) return MSV_ERR_INVALID_ARGUMENT;
    if (residues_len >= (1ull << 32) || n >= kMaxLaunchSeqs) return MSV_ERR_INVALID_ARGUMENT;
    DeviceGuard g(p->device);
    if (!g.ok) return MSV_ERR_NO_DEVICE;
    hipStream_t st = stream ? static_cast<hipStream_t>(stream) : p->stream;

    const Plan& plan = select_plan(p, n, latency_ok, host_residues);
    msvk::KernelArgs a = kernel_args(p, plan, d_residues, residues_len, d_offsets, n, d_order, d_scores);
    if (d_errors) a.errors = d_errors;
    const bool clock = p->stamp_clock && !host_residues;
    a.stamps = p->d_stamps;
    if (p->stamp_clock && (plan.cv || !plan.v->clock_fn || host_residues)) a.stamps = nullptr;  // no CLOCK twin

    const uint64_t want = (n + plan.groups_per_block - 1) / plan.groups_per_block;
    const int blocks = static_cast<int>(std::min<uint64_t>(static_cast<uint64_t>(plan.blocks), want));
    hipEvent_t t0 = p->time_start, t1 = p->time_stop;
    p->time_start = p->time_stop = nullptr;
    if (plan.cv) {  // the cooperative plan: a workgroup per sequence, no dequeue counter
        void* params[] = {&a};
        const dim3 block(static_cast<uint32_t>(plan.cv->waves * 64));
        MSV_HIP(t0 || t1 ? hipExtLaunchKernel(plan.cv->fn, dim3(blocks), block, params, 0, st, t0, t1, 0)
                         : hipLaunchKernel(plan.cv->fn, dim3(blocks), block, params, 0, st));
        return MSV_OK;
    }
    // the twin of a residue-block variant (rows of <= 40 states) reads 4-byte superblock words, clamped
    // to the buffer only from 4 bytes up: it takes buffers of at least 64 bytes
    const bool wide = plan.v->S <= 40;  // (twins of rows > 40 states prefetch two rows; see zc_fn)
    const bool twin = host_residues && (!wide || (p->zc_wide && residues_len >= 64));
    // A slot's counters (next index, waves left) are zero between launches: zeroed at creation and
    // put back by the last wave of every launch (msv_kernel.hip).  A failed launch may leave them
    // dirty, so the slot's next launch resets them explicitly (LaunchRing::run).
    MSV_HIP(p->kernels.run(st, lazy_stream(p, st), p->d_words.get(), 2, [&](uint32_t* counter) {
        a.counter = counter;
        return msvk::launch_variant(*plan.v, dim3(blocks), a, st, t0, t1, twin, clock);
    }));
    return MSV_OK;
}

msv_status msv_score_batch_device(msv_profile* p, const uint8_t* d_residues, uint64_t residues_len,
                                  const uint64_t* d_offsets, uint64_t n, const uint32_t* d_order, float* d_scores,
                                  void* stream) {
    return launch_batch(p, d_residues, residues_len, d_offsets, n, d_order, d_scores, stream, true);
}

// Library-internal (msv_multi.cpp): msv_score_batch_device for residues that are the device alias of
// page-locked host memory -- the launch takes the variant's zero-copy twin (msv_kernel.hip zc_fn).
__attribute__((visibility("hidden"))) msv_status msv_score_batch_host_residues(
    msv_profile* p, const uint8_t* d_residues, uint64_t residues_len, const uint64_t* d_offsets, uint64_t n,
    const uint32_t* d_order, float* d_scores, void* stream) {
    return launch_batch(p, d_residues, residues_len, d_offsets, n, d_order, d_scores, stream, true, nullptr, true);
}

msv_status msv_profile_bind_stream(msv_profile* p, void* stream) {
    if (!p) return MSV_ERR_INVALID_ARGUMENT;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (st == p->bound) return MSV_OK;
    DeviceGuard g(p->device);
    if (!g.ok) return MSV_ERR_NO_DEVICE;
    if (p->bound) {  // the old stream loses its guarantee: record what is still pending on it
        MSV_HIP(p->kernels.flush(p->bound));
        MSV_HIP(p->orders.flush(p->bound));
    }
    p->bound = st;
    return MSV_OK;
}

// Synchronises `st`, then reads, clears and reports error word `word` of the profile.
static msv_status check_word(msv_profile* p, hipStream_t st, int word) {
    uint32_t err = 0;
    MSV_HIP(hipMemcpyAsync(&err, p->d_words + word, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    MSV_HIP(hipStreamSynchronize(st));
    if (err) MSV_HIP(hipMemsetAsync(p->d_words + word, 0, sizeof(uint32_t), st));
    MSV_HIP(hipStreamSynchronize(st));
    return err_status(err);
}

// The status of a finished batch whose `n` scores are on the host, with `st` idle.  Every error leaves a score
// that is +inf or NaN (scan_scores), so the latched error words are read back only on that rare path (a 4-byte
// read-back is a blit launch plus a synchronisation: 4 us per call, 0.9 ms over a grid's 24 profiles, more
// than its kernels): then word `word` of EVERY listed profile is read and cleared, the first status reported.
static msv_status host_scores_status(const float* scores, uint64_t n, msv_profile* const* profiles, uint32_t n_profiles,
                                     hipStream_t st, int word) {
    if (scan_scores(scores, n) == MSV_OK) return MSV_OK;
    msv_status first = MSV_OK;
    for (uint32_t i = 0; i < n_profiles; ++i) {
        const msv_status s = check_word(profiles[i], st, word);
        if (first == MSV_OK) first = s;
    }
    return first != MSV_OK ? first : scan_scores(scores, n);
}

msv_status msv_profile_check(msv_profile* p, void* stream) {
    if (!p) return MSV_ERR_INVALID_ARGUMENT;
    DeviceGuard g(p->device);
    if (!g.ok) return MSV_ERR_NO_DEVICE;
    return check_word(p, stream ? static_cast<hipStream_t>(stream) : p->stream, kErrWord);
}

msv_status msv_order_longest_first(msv_profile* p, const uint64_t* d_offsets, uint64_t n, uint32_t* d_order,
                                   void* stream) {
    if (!p || (n && (!d_offsets || !d_order))) return MSV_ERR_INVALID_ARGUMENT;
    if (n == 0) return MSV_OK;
    DeviceGuard g(p->device);
    if (!g.ok) return MSV_ERR_NO_DEVICE;
    hipStream_t st = stream ? static_cast<hipStream_t>(stream) : p->stream;
    constexpr size_t kScratch = msvk::kOrderScratchWords(kOrderBins);
    if (!p->d_hist) {
        MSV_HIP(p->d_hist.reserve(kLaunchSlots * kScratch));
        std::fill(std::begin(p->orders.dirty), std::end(p->orders.dirty), true);  // fresh memory
    }
    // [histogram | cursors | ticket] per slot; the sort leaves histogram and ticket zeroed for the slot's next use
    MSV_HIP(p->orders.run(st, lazy_stream(p, st), p->d_hist.get(), kScratch, [&](uint32_t* scratch) {
        return msvk::launch_order(d_offsets, n, scratch, kOrderBins, d_order, st);
    }));
    return MSV_OK;
}

msv_status msv_host_alloc(size_t bytes, void** out) {
    if (!out) return MSV_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    MSV_HIP(hipHostMalloc(out, std::max<size_t>(bytes, 1), hipHostMallocPortable));
    return MSV_OK;
}

msv_status msv_host_free(void* ptr) {
    if (ptr) MSV_HIP(hipHostFree(ptr));
    return MSV_OK;
}

msv_status msv_score_batch(msv_profile* p, const uint8_t* residues, const uint64_t* offsets, uint64_t n,
                           float* scores, void* stream) {
    // 1. validate: the CSR on the host (cheap, O(n)), and find the longest sequence
    if (!p || (n && (!offsets || !scores))) return MSV_ERR_INVALID_ARGUMENT;
    if (n == 0) return MSV_OK;
    uint64_t maxL = 0, total = 0;
    msv_status s = csr_extent(offsets, n, &maxL, &total);
    if (s != MSV_OK) return s;
    if (maxL >= kChunkBytes) return MSV_ERR_SEQUENCE_TOO_LONG;
    if (total && !residues) return MSV_ERR_INVALID_ARGUMENT;
    s = msv_profile_reserve_length(p, maxL);
    if (s != MSV_OK) return s;

    DeviceGuard g(p->device);
    if (!g.ok) return MSV_ERR_NO_DEVICE;
    hipStream_t st = stream ? static_cast<hipStream_t>(stream) : p->stream;

    // 2. plan (msv_plan.h plan_call): how the residues reach the kernels, the pieces, the staging layout.
    // IN PLACE.  Page-locked residues are not copied at all: the kernel reads them in place over PCIe through
    // their device alias (zero-copy; L2 keeps each 128-B line for the rows that follow).  cfg3: kernel 2.98 vs
    // 2.87 ms from HBM -- 0.96 of the resident rate with no copy, against ~0.85 for the copy pipeline
    // below, whose first piece's copy and extra drain tail it saves (profiles/r02_zero_copy_probe.jsonl).
    // One launch per < 2^32-byte piece; no copy stream, no second compute stream.
    // Except for large batches of small models (in_place_wins), whose kernel consumes residues faster than the
    // ~25 GB/s at which a kernel reads host memory: page-locked 100k x U[300,500] batches, per call in place vs
    // copied (profiles/r03_ab_in_place_vs_copied.jsonl): 100.hmm 1.60 vs 1.24 ms, 200.hmm 1.69 vs 1.46, 400.hmm
    // 1.68 vs 1.76, 600.hmm 1.75 vs 2.33, 1400.hmm 3.09 vs 3.36; 100.hmm x 20k (8 MB) 0.41 vs 0.44.
    // SMALL calls: the residues ride in the offsets' H2D (behind the n + 1 offsets, in u64 words), and
    // pageable scores are written by the kernel into pinned staging.  A one-sequence call was two H2D
    // and two D2H blits, the scores' D2H to pageable memory a ~25 us round trip on the host
    // (profiles/r03_reference_call_timeline.txt).
    // COPIED, as a copy/compute pipeline from kPipelineMin residues up.  The batch is cut into pieces
    // (contiguous sequence ranges) whose residue counts grow geometrically from 1/4 of the batch (x2: 2 pieces
    // for cfg3, the best plan in tools/host_pipeline_sweep.py, profiles/r02_host_pipeline_sweep.jsonl), so the
    // first kernel starts after a short copy and every later piece's H2D (copy stream) runs under the kernels
    // of the pieces before it.
    const uint8_t* const zres = (total && p->zero_copy && msvplan::in_place_wins(p->model_length - 1, total))
                                    ? mapped_host(residues) : nullptr;
    const CallPlan plan = msvplan::plan_call(offsets, n, total, zres != nullptr, p->pipe_first_den, p->pipe_growth);
    const std::vector<uint64_t>& cut = plan.cut;
    const size_t P = plan.pieces();
    const bool in_place = plan.mode == CallPlan::kInPlace, small = plan.mode == CallPlan::kSmall, pipe = plan.pipeline;
    // 3. reserve.  A page-locked destination is written by the kernels themselves (no D2H of the scores);
    // the offsets' pinned staging also holds the small call's residues and the error word (plan's layout).
    CsrStaging& sg = p->host;
    float* direct = mapped_host(scores);
    const bool staged_scores = !direct && small;
    if (staged_scores) {
        MSV_HIP(p->h_sc.reserve(std::max<uint64_t>(n, 64), hipHostMallocDefault));
        direct = mapped_host(p->h_sc.get());
        if (!direct) return MSV_ERR_HIP;
    }
    MSV_HIP(sg.reserve_inputs(plan.staged_words(), plan.mode == CallPlan::kCopied ? total : 0));
    MSV_HIP(sg.reserve_results(n, direct ? 0 : n));
    float* const dsc = direct ? direct : sg.d_scores.get();
    uint32_t* const h_err = reinterpret_cast<uint32_t*>(sg.h_off + plan.err_word());
    const uint8_t* const d_small_res = reinterpret_cast<const uint8_t*>(sg.d_off + plan.small_res_word());

    // 4. fork: the pipeline's copy stream and second compute stream start after the caller's stream's
    // earlier work.  On an early error return, copies reading the pinned h_off (rewritten by the next call)
    // and kernels writing the staging buffers may still be queued: drain every stream used first.
    hipStream_t cs[2] = {st, st}, cp = st;
    if (pipe) {
        MSV_HIP(p->stream2.create(hipStreamNonBlocking));
        MSV_HIP(p->copy_stream.create(hipStreamNonBlocking));
        cs[1] = p->pipe_streams == 2 ? p->stream2 : st;
        cp = p->copy_stream;
    }
    StreamDrain drain(cs[0], cs[1], cp);
    if (pipe) {
        while (p->events.size() < P + 4) {
            msvrt::Event e;
            MSV_HIP(e.create(hipEventDisableTiming | hipEventReleaseToDevice));
            p->events.push_back(std::move(e));
        }
        MSV_HIP(hipEventRecord(p->events[P + 2], st));
        MSV_HIP(hipStreamWaitEvent(cp, p->events[P + 2], 0));
        MSV_HIP(hipStreamWaitEvent(cs[1], p->events[P + 2], 0));
    }
    // 5. the residue pieces go first, in order, on the copy stream: their DMA is the critical path
    for (size_t k = 0; k < P; ++k) {
        const uint64_t at = offsets[cut[k]], bytes = offsets[cut[k + 1]] - at;
        if (bytes && plan.mode == CallPlan::kCopied)
            MSV_HIP(hipMemcpyAsync(sg.d_res + (at - offsets[0]), residues + at, bytes, hipMemcpyHostToDevice, cp));
        if (pipe) MSV_HIP(hipEventRecord(p->events[2 + k], cp));  // piece k's residues landed
    }
    // 6. meanwhile every piece's offsets (rebased on the piece's first residue, at plan.offsets_word(k))
    //    in ONE H2D on the caller's stream, then every piece's longest-first order there, before the first
    //    kernel and under the first residue copy (an order kernel enqueued behind a running MSV kernel would
    //    find no free VGPRs until that kernel's blocks drain, delaying the next piece's launch)
    for (size_t k = 0; k < P; ++k) msvplan::rebase_offsets(offsets, cut[k], cut[k + 1], sg.h_off + plan.offsets_word(k));
    if (small && total) std::memcpy(sg.h_off + plan.small_res_word(), residues + offsets[0], total);
    MSV_HIP(hipMemcpyAsync(sg.d_off, sg.h_off, plan.upload_words() * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    const bool sort = pipe || !order_needless(p, n, in_place);
    for (size_t k = 0; k < P && sort; ++k) {
        s = msv_order_longest_first(p, sg.d_off + plan.offsets_word(k), cut[k + 1] - cut[k], sg.d_order + cut[k], st);
        if (s != MSV_OK) return s;
    }
    if (pipe) {
        MSV_HIP(hipEventRecord(p->events[1], st));  // offsets and orders done
        MSV_HIP(hipStreamWaitEvent(cs[1], p->events[1], 0));
    }
    // 7. the kernels, each after its piece's residues.  Pieces alternate over the two compute streams, so a
    //    piece's kernel fills the CUs that the previous piece's drain tail frees (each launch has its own
    //    dequeue counter slot), and so that the LAST piece runs on the caller's stream (the scores' D2H then
    //    waits on no other stream).
    for (size_t k = 0; k < P; ++k) {
        const uint64_t at = offsets[cut[k]], bytes = offsets[cut[k + 1]] - at;
        hipStream_t c = cs[(P - 1 - k) & 1];
        if (pipe) MSV_HIP(hipStreamWaitEvent(c, p->events[2 + k], 0));
        const uint8_t* src = in_place ? zres + at : (small ? d_small_res : sg.d_res.get()) + (at - offsets[0]);
        s = launch_batch(p, sg.readable(src, bytes), std::max<uint64_t>(bytes, 1), sg.d_off + plan.offsets_word(k),
                         cut[k + 1] - cut[k], sort ? sg.d_order + cut[k] : nullptr, dsc + cut[k], c, !pipe,
                         p->d_words + kHostErrWord, in_place && bytes);
        if (s != MSV_OK) return s;
    }
    // 8. join the second compute stream (done before the last piece) back into the caller's
    if (pipe) {
        MSV_HIP(hipEventRecord(p->events[P + 3], cs[1]));
        MSV_HIP(hipStreamWaitEvent(st, p->events[P + 3], 0));
    }
    // 9. finish.  Scores and the error word come back once at the end (pageable destinations would make
    //    per-piece D2H copies block the host thread that enqueues the pipeline), followed by ONE
    //    synchronisation (also: the pinned h_off is rewritten by the next call).
    if (!direct) {
        MSV_HIP(hipMemcpyAsync(scores, sg.d_scores, n * sizeof(float), hipMemcpyDeviceToHost, st));
        MSV_HIP(hipMemcpyAsync(h_err, p->d_words + kHostErrWord, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    }
    MSV_HIP(hipStreamSynchronize(st));
    drain.disarm();
    if (!direct) return *h_err == 0 ? MSV_OK : check_word(p, st, kHostErrWord);  // reads, clears, reports its bits
    if (staged_scores) std::memcpy(scores, p->h_sc, n * sizeof(float));
    return host_scores_status(scores, n, &p, 1, st, kHostErrWord);  // (scores in page-locked memory)
}

msv_status msv_score_batch_async(msv_profile* p, const uint8_t* residues, const uint64_t* offsets, uint64_t n,
                                 float* scores, uint64_t* ticket) {
    if (!p || !ticket || (n && (!offsets || !scores))) return MSV_ERR_INVALID_ARGUMENT;
    *ticket = 0;
    uint64_t maxL = 0, total = 0;
    msv_status s = csr_extent(offsets, n, &maxL, &total);
    if (s != MSV_OK) return s;
    if (total && !residues) return MSV_ERR_INVALID_ARGUMENT;
    // one launch per call: split larger batches (or use msv_score_batch)
    if (total >= kChunkBytes || n >= kMaxLaunchSeqs) return MSV_ERR_INVALID_ARGUMENT;
    auto& a = p->async[p->next_ticket % kAsyncSlots];
    if (a.pending) return MSV_ERR_INVALID_ARGUMENT;  // that slot's call has not been waited for
    s = msv_profile_reserve_length(p, maxL);
    if (s != MSV_OK) return s;
    DeviceGuard g(p->device);
    if (!g.ok) return MSV_ERR_NO_DEVICE;
    MSV_HIP(p->copy_stream.create(hipStreamNonBlocking));
    MSV_HIP(p->offsets_stream.create(hipStreamNonBlocking));
    MSV_HIP(a.copied.create(hipEventDisableTiming));
    MSV_HIP(a.off_copied.create(hipEventDisableTiming));
    MSV_HIP(a.done.create(hipEventDisableTiming));
    MSV_HIP(a.h_err.reserve(64 / sizeof(uint32_t), hipHostMallocDefault));
    CsrStaging& sg = a.staged;
    float* const direct = n ? mapped_host(scores) : nullptr;
    MSV_HIP(sg.reserve_results(n, direct ? 0 : std::max<uint64_t>(n, 1)));
    const int slot = static_cast<int>(&a - p->async);
    uint32_t* d_err = p->d_words + kErrWord + 1 + slot;
    // Consecutive calls alternate over two compute streams, so a call's kernel fills the CUs that the
    // previous call's drain tail frees instead of starting after the whole previous kernel.
    const bool odd = (p->next_ticket & 1) != 0;
    if (odd) MSV_HIP(p->stream2.create(hipStreamNonBlocking));
    hipStream_t cp = p->copy_stream, co = p->offsets_stream, cs = odd ? p->stream2 : p->stream;
    // On an error return after the first enqueue, copies reading this slot's pinned offsets (rewritten by
    // the slot's next call) may still be queued: drain the call's streams first.
    StreamDrain drain(co, cp, cs);
    // copy streams: this call's inputs (they overlap the earlier calls' kernels on the compute streams).
    // Nothing but copies goes on them: a kernel there (the order, as in round 2) waits for the running MSV
    // grid to drain before it can start, and every later call's copies queued behind it.  The offsets
    // have a stream of their own, so the copy stream carries the residues back to back (cfg2: 83 us
    // each, which set the call rate with the offsets' 8 us copy and the gaps between them in the same
    // stream -- profiles/r03_cfg2_streamed_timeline.txt) and the order starts once the offsets land.
    MSV_HIP(sg.upload(residues, offsets, 0, n, true, co, cp));
    MSV_HIP(hipEventRecord(a.off_copied, co));
    MSV_HIP(hipEventRecord(a.copied, cp));
    // compute stream: order, kernel, scores and the slot's error word back to the host (the order runs
    // in the previous call's drain tail: that call's kernel is on the other compute stream)
    MSV_HIP(hipStreamWaitEvent(cs, a.off_copied, 0));
    const bool sort = n && !order_needless(p, n, false);
    if (sort) {
        s = msv_order_longest_first(p, sg.d_off, n, sg.d_order, cs);
        if (s != MSV_OK) return s;
    }
    MSV_HIP(hipStreamWaitEvent(cs, a.copied, 0));
    if (n) {
        s = launch_batch(p, sg.readable(sg.d_res, total), std::max<uint64_t>(total, 1), sg.d_off, n,
                         sort ? sg.d_order.get() : nullptr, direct ? direct : sg.d_scores.get(), cs, true, d_err);
        if (s != MSV_OK) return s;
        if (!direct) MSV_HIP(hipMemcpyAsync(scores, sg.d_scores, n * sizeof(float), hipMemcpyDeviceToHost, cs));
    }
    if (!direct) {  // (direct: errors are read from the scores; nothing else follows the kernel)
        MSV_HIP(hipMemcpyAsync(a.h_err, d_err, sizeof(uint32_t), hipMemcpyDeviceToHost, cs));
        MSV_HIP(hipMemsetAsync(d_err, 0, sizeof(uint32_t), cs));
    }
    MSV_HIP(hipEventRecord(a.done, cs));
    drain.disarm();
    a.direct = direct ? scores : nullptr;
    a.n = n;
    a.ticket = p->next_ticket++;
    a.pending = true;
    *ticket = a.ticket;
    return MSV_OK;
}

msv_status msv_profile_wait(msv_profile* p, uint64_t ticket) {
    if (!p || ticket == 0) return MSV_ERR_INVALID_ARGUMENT;
    for (auto& a : p->async) {
        if (!a.pending || a.ticket != ticket) continue;
        DeviceGuard g(p->device);
        if (!g.ok) return MSV_ERR_NO_DEVICE;
        MSV_HIP(hipEventSynchronize(a.done));
        a.pending = false;
        // (direct: classified from the bits the kernel latched in the slot's error word, cleared there)
        if (a.direct)
            return host_scores_status(a.direct, a.n, &p, 1, p->stream, kErrWord + 1 + static_cast<int>(&a - p->async));
        return err_status(*a.h_err);
    }
    return MSV_ERR_INVALID_ARGUMENT;  // unknown ticket, or already waited for
}

// The plan of `p` whose table is in variant v's layout (installing it as p->fused if none is).
static msv_status plan_in_layout(msv_profile* p, const msvk::Variant* v, const Plan** out) {
    for (const Plan* q : {&p->main, &p->lat, &p->mid, &p->fused})
        if (q->v == v) {
            *out = q;
            return MSV_OK;
        }
    const msv_status s = install_plan(p, v, p->fused);
    if (s != MSV_OK) return s;
    *out = &p->fused;
    return MSV_OK;
}

// The plan of `p` whose table is in cooperative variant cv's layout (installing it as p->coop_fused).
static msv_status coop_plan_in_layout(msv_profile* p, const msvk::CoopVariant* cv, const Plan** out) {
    for (const Plan* q : {&p->coop, &p->coop_fused})
        if (q->cv == cv) {
            *out = q;
            return MSV_OK;
        }
    const msv_status s = install_coop_table(p, cv, p->coop_fused);
    if (s != MSV_OK) return s;
    *out = &p->coop_fused;
    return MSV_OK;
}

// How a grid of n sequences x these profiles runs (msv_plan.h fused_grid).
static msvplan::GridChoice grid_choice(msv_profile* const* profiles, uint32_t n_profiles, uint64_t n,
                                       bool host_residues) {
    std::vector<msvplan::GridProfile> shapes(n_profiles);
    uint32_t most = 0;  // the most times one handle is listed
    for (uint32_t i = 0; i < n_profiles; ++i) {
        const msv_profile* p = profiles[i];
        shapes[i] = {p->model_length - 1, p->force, std::memcmp(&p->tr_E_C, &p->tr_E_J, sizeof(float)) == 0,
                     p->chosen.coop_max_n};
        uint32_t same = 0;
        for (uint32_t j = 0; j < n_profiles; ++j) same += profiles[j] == p;
        most = std::max(most, same);
    }
    return msvplan::fused_grid(plan_tables(), shapes.data(), n_profiles, n, host_residues, most);
}

// A grid of few sequences on the cooperative plan: ONE msv_coop_grid_kernel launch per 32 profiles, every
// profile's table in the cooperative layout of the grid's largest model, one workgroup per (profile,
// sequence).  The whole grid then lasts about as long as one sequence on one profile: benchmark_MSV's
// 24 profiles x 3 sequences of 3,500 residues run as 72 workgroups at once.  No dequeue counters.
static msv_status grid_coop_fused(msv_profile* const* profiles, uint32_t n_profiles, const msvk::CoopVariant* cv,
                                  const uint8_t* d_residues, uint64_t residues_len, const uint64_t* d_offsets,
                                  uint64_t n, const uint32_t* d_order, float* d_scores, hipStream_t cs) {
    if (residues_len >= (1ull << 32) || !d_offsets || (residues_len && !d_residues)) return MSV_ERR_INVALID_ARGUMENT;
    for (uint32_t first = 0; first < n_profiles; first += msvk::kGridMaxProfiles) {
        const uint32_t count = std::min(n_profiles - first, msvk::kGridMaxProfiles);
        msvk::GridArgs ga{};
        ga.profiles = count;
        ga.per_profile = static_cast<uint32_t>(n);
        for (uint32_t j = 0; j < count; ++j) {
            msv_profile* p = profiles[first + j];
            const Plan* plan = nullptr;
            const msv_status s = coop_plan_in_layout(p, cv, &plan);
            if (s != MSV_OK) return s;
            ga.p[j] = kernel_args(p, *plan, d_residues, residues_len, d_offsets, n, d_order,
                                  d_scores + static_cast<uint64_t>(first + j) * n);
        }
        void* params[] = {&ga};
        MSV_HIP(hipLaunchKernel(cv->grid_fn, dim3(count * ga.per_profile), dim3(static_cast<uint32_t>(cv->waves * 64)),
                                params, 0, cs));
    }
    return MSV_OK;
}

static msv_status grid_fused(msv_profile* const* profiles, uint32_t n_profiles, const msvk::Variant* v,
                             const uint8_t* d_residues, uint64_t residues_len, const uint64_t* d_offsets, uint64_t n,
                             const uint32_t* d_order, float* d_scores, hipStream_t cs) {
    if (residues_len >= (1ull << 32) || !d_offsets || (residues_len && !d_residues)) return MSV_ERR_INVALID_ARGUMENT;
    const uint32_t groups_per_block = static_cast<uint32_t>(v->waves * (64 / v->G) * v->streams);
    for (uint32_t first = 0; first < n_profiles; first += msvk::kGridMaxProfiles) {
        const uint32_t count = std::min(n_profiles - first, msvk::kGridMaxProfiles);
        msvk::GridArgs ga{};
        ga.profiles = count;
        ga.per_profile = static_cast<uint32_t>((n + groups_per_block - 1) / groups_per_block);
        int slot[msvk::kGridMaxProfiles];
        for (uint32_t j = 0; j < count; ++j) {
            msv_profile* p = profiles[first + j];
            const Plan* plan = nullptr;
            msv_status s = plan_in_layout(p, v, &plan);
            if (s != MSV_OK) return s;
            msvk::KernelArgs& a = ga.p[j];
            a = kernel_args(p, *plan, d_residues, residues_len, d_offsets, n, d_order,
                            d_scores + static_cast<uint64_t>(first + j) * n);
            MSV_HIP(p->kernels.acquire(cs, &slot[j]));
            a.counter = p->d_words + 2 * slot[j];
            if (p->kernels.dirty[slot[j]]) MSV_HIP(hipMemsetAsync(a.counter, 0, 2 * sizeof(uint32_t), cs));
            p->kernels.dirty[slot[j]] = true;
        }
        MSV_HIP(msvk::launch_grid_variant(*v, ga, cs));
        for (uint32_t j = 0; j < count; ++j) {
            msv_profile* p = profiles[first + j];
            p->kernels.dirty[slot[j]] = false;
            MSV_HIP(p->kernels.release(slot[j], cs, lazy_stream(p, cs)));
        }
    }
    return MSV_OK;
}

// host_residues: d_residues is the device alias of page-locked host memory (msv_score_grid's in-place
// read): no cooperative plan (fused or per profile) and the per-profile launches take the zero-copy twins.
static msv_status score_grid_device(msv_profile* const* profiles, uint32_t n_profiles, const uint8_t* d_residues,
                                    uint64_t residues_len, const uint64_t* d_offsets, uint64_t n,
                                    const uint32_t* d_order, float* d_scores, void* stream, bool host_residues) {
    if (!profiles || n_profiles == 0) return MSV_ERR_INVALID_ARGUMENT;
    for (uint32_t i = 0; i < n_profiles; ++i)
        if (!profiles[i] || profiles[i]->device != profiles[0]->device) return MSV_ERR_INVALID_ARGUMENT;
    if (n == 0) return MSV_OK;
    if (!d_scores) return MSV_ERR_INVALID_ARGUMENT;
    DeviceGuard g(profiles[0]->device);
    if (!g.ok) return MSV_ERR_NO_DEVICE;
    hipStream_t cs = stream ? static_cast<hipStream_t>(stream) : profiles[0]->stream;
    const msvplan::GridChoice fused = grid_choice(profiles, n_profiles, n, host_residues);
    int count = 0;
    if (fused.kind == msvplan::GridChoice::kCoopFused)
        return grid_coop_fused(profiles, n_profiles, &msvk::coop_variants(&count)[fused.index], d_residues, residues_len,
                               d_offsets, n, d_order, d_scores, cs);
    if (fused.kind == msvplan::GridChoice::kLatencyFused)
        return grid_fused(profiles, n_profiles, &msvk::variants(&count)[fused.index], d_residues, residues_len,
                          d_offsets, n, d_order, d_scores, cs);
    msvrt::Event fork;
    MSV_HIP(fork.create(hipEventDisableTiming));
    MSV_HIP(hipEventRecord(fork, cs));
    // Largest models first: their launches are the longest, and with more streams than hardware queues
    // (HIP's default is 4) the launches queued behind them are the short ones.
    std::vector<uint32_t> launch_order(n_profiles);
    for (uint32_t i = 0; i < n_profiles; ++i) launch_order[i] = i;
    std::stable_sort(launch_order.begin(), launch_order.end(), [&](uint32_t x, uint32_t y) {
        return profiles[x]->model_length > profiles[y]->model_length;
    });
    for (const uint32_t i : launch_order) {
        msv_profile* p = profiles[i];
        MSV_HIP(p->done.create(hipEventDisableTiming));
        hipStream_t ps = p->stream == cs ? cs : p->stream;
        if (ps != cs) MSV_HIP(hipStreamWaitEvent(ps, fork, 0));
        const msv_status s = launch_batch(p, d_residues, residues_len, d_offsets, n, d_order,
                                          d_scores + static_cast<uint64_t>(i) * n, ps, true, nullptr, host_residues);
        if (s != MSV_OK) return s;
        if (ps != cs) {
            MSV_HIP(hipEventRecord(p->done, ps));
            MSV_HIP(hipStreamWaitEvent(cs, p->done, 0));
        }
    }
    return MSV_OK;
}

msv_status msv_score_grid_device(msv_profile* const* profiles, uint32_t n_profiles, const uint8_t* d_residues,
                                 uint64_t residues_len, const uint64_t* d_offsets, uint64_t n,
                                 const uint32_t* d_order, float* d_scores, void* stream) {
    return score_grid_device(profiles, n_profiles, d_residues, residues_len, d_offsets, n, d_order, d_scores, stream,
                             false);
}

msv_status msv_score_grid(msv_profile* const* profiles, uint32_t n_profiles, const uint8_t* residues,
                          const uint64_t* offsets, uint64_t n, float* scores, void* stream) {
    if (!profiles || n_profiles == 0 || (n && (!offsets || !scores))) return MSV_ERR_INVALID_ARGUMENT;
    for (uint32_t i = 0; i < n_profiles; ++i)
        if (!profiles[i] || profiles[i]->device != profiles[0]->device) return MSV_ERR_INVALID_ARGUMENT;
    if (n == 0) return MSV_OK;
    uint64_t maxL = 0, bytes = 0;
    msv_status s = csr_extent(offsets, n, &maxL, &bytes);
    if (s != MSV_OK) return s;
    if (bytes && !residues) return MSV_ERR_INVALID_ARGUMENT;
    if (bytes >= kChunkBytes || n >= kMaxLaunchSeqs) {  // huge batch: per profile, chunked
        for (uint32_t i = 0; i < n_profiles; ++i) {
            s = msv_score_batch(profiles[i], residues, offsets, n, scores + i * n, stream);
            if (s != MSV_OK) return s;
        }
        return MSV_OK;
    }
    for (uint32_t i = 0; i < n_profiles; ++i) {
        s = msv_profile_reserve_length(profiles[i], maxL);
        if (s != MSV_OK) return s;
    }
    msv_profile* p0 = profiles[0];
    DeviceGuard g(p0->device);
    if (!g.ok) return MSV_ERR_NO_DEVICE;
    hipStream_t st = stream ? static_cast<hipStream_t>(stream) : shared_stream(p0->device);
    if (!st) st = p0->stream;
    if (!stream)
        for (uint32_t i = 0; i < n_profiles; ++i) profiles[i]->shared = st;  // lazy slot events (lazy_stream)
    // The first profile's staging buffers (a host call is synchronous, like msv_score_batch's use of
    // them): per-call hipMalloc/hipFree of four buffers cost more than the kernels of a small grid.
    // Page-locked residues are read in place and a page-locked destination is written by the kernels,
    // as in msv_score_batch.
    const uint64_t total = static_cast<uint64_t>(n_profiles) * n;
    CsrStaging& sg = p0->host;
    const uint8_t* const zbase = (bytes && p0->zero_copy) ? mapped_host(residues) : nullptr;
    const uint8_t* const zres = zbase ? zbase + offsets[0] : nullptr;
    float* const direct = mapped_host(scores);
    MSV_HIP(sg.reserve_results(n, direct ? 0 : total));
    // an early error return leaves nothing queued that reads h_off or the staging buffers
    StreamDrain drain(st);
    MSV_HIP(sg.upload(residues, offsets, 0, n, !zres, st, st));
    const uint8_t* d_res = zres ? zres : sg.d_res.get();
    // (a fused cooperative grid runs one workgroup per sequence: no dequeue order to sort; residues read
    // in place never take it)
    const bool sort = grid_choice(profiles, n_profiles, n, zres != nullptr).kind != msvplan::GridChoice::kCoopFused;
    s = sort ? msv_order_longest_first(p0, sg.d_off, n, sg.d_order, st) : MSV_OK;
    if (s != MSV_OK) return s;
    float* const dsc = direct ? direct : sg.d_scores.get();
    s = score_grid_device(profiles, n_profiles, sg.readable(d_res, bytes), std::max<uint64_t>(bytes, 1), sg.d_off, n,
                          sort ? sg.d_order.get() : nullptr, dsc, st, zres != nullptr);
    if (s != MSV_OK) return s;
    if (!direct) MSV_HIP(hipMemcpyAsync(scores, sg.d_scores, total * sizeof(float), hipMemcpyDeviceToHost, st));
    drain.disarm();
    MSV_HIP(hipStreamSynchronize(st));  // pageable host buffers above
    // (the grid's launches latch their errors in the profiles' device-launch words)
    return host_scores_status(scores, total, profiles, n_profiles, st, kErrWord);
}

// Host restatement of msvk::msv_pvalue_of (kept textually parallel; tests compare both).
static double host_pvalue(float score, uint64_t L, float mu, float lambda) {
    if (L == 0) return 1.0;  // empty sequence: score -inf, and L log(p1) would be 0 * -inf
    const float p1 = static_cast<float>(L) / static_cast<float>(L + 1);
    const float nullsc = static_cast<float>(static_cast<double>(L) * std::log(static_cast<double>(p1)) +
                                            std::log(1.0 - static_cast<double>(p1)));
    const float bits = (score - nullsc) / 0.69314718055994529f;
    const double y = static_cast<double>(lambda) * (static_cast<double>(bits) - static_cast<double>(mu));
    const double ey = -std::exp(-y);
    return std::fabs(ey) < 5e-9 ? -ey : 1.0 - std::exp(ey);
}

msv_status msv_pvalues(const float* scores, const uint64_t* offsets, uint64_t n, float mu, float lambda,
                       double* pvalues) {
    if (n && (!scores || !offsets || !pvalues)) return MSV_ERR_INVALID_ARGUMENT;
    for (uint64_t i = 0; i < n; ++i) {
        if (offsets[i + 1] < offsets[i]) return MSV_ERR_INVALID_ARGUMENT;
        pvalues[i] = host_pvalue(scores[i], offsets[i + 1] - offsets[i], mu, lambda);
    }
    return MSV_OK;
}

msv_status msv_pvalues_device(int device, const float* d_scores, const uint64_t* d_offsets, uint64_t n, float mu,
                              float lambda, double* d_pvalues, void* stream) {
    if (n == 0) return MSV_OK;
    if (!d_scores || !d_offsets || !d_pvalues) return MSV_ERR_INVALID_ARGUMENT;
    DeviceGuard g(device);
    if (!g.ok) return MSV_ERR_NO_DEVICE;
    MSV_HIP(msvk::launch_pvalues(d_scores, d_offsets, n, mu, lambda, d_pvalues, static_cast<hipStream_t>(stream)));
    return MSV_OK;
}

msv_status msv_score_batch_multi(msv_profile* const* profiles, uint32_t n_profiles, const uint8_t* residues,
                                 const uint64_t* offsets, uint64_t n, float* scores) {
    if (!profiles || n_profiles == 0 || (n && (!offsets || !scores))) return MSV_ERR_INVALID_ARGUMENT;
    for (uint32_t k = 0; k < n_profiles; ++k)
        if (!profiles[k]) return MSV_ERR_INVALID_ARGUMENT;
    if (n == 0) return MSV_OK;
    std::vector<uint64_t> b(n_profiles + 1);
    msv_status s = msv_shard_bounds(offsets, n, n_profiles, b.data());
    if (s != MSV_OK) return s;
    // One host thread per DISTINCT profile handle: a handle listed more than once scores its shards
    // one after another on its thread (a profile's staging buffers and streams serve one host
    // thread at a time).
    std::vector<msv_status> st(n_profiles, MSV_OK);
    std::vector<std::thread> workers;
    for (uint32_t k = 0; k < n_profiles; ++k) {
        bool first_use = true;
        for (uint32_t j = 0; j < k; ++j) first_use = first_use && profiles[j] != profiles[k];
        if (!first_use) continue;
        workers.emplace_back([&, k] {
            for (uint32_t j = k; j < n_profiles && st[k] == MSV_OK; ++j) {
                if (profiles[j] != profiles[k] || b[j + 1] == b[j]) continue;
                // offsets stay absolute: msv_score_batch rebases every piece on its first offset
                st[k] = msv_score_batch(profiles[k], residues, offsets + b[j], b[j + 1] - b[j], scores + b[j], nullptr);
            }
        });
    }
    for (auto& w : workers) w.join();
    for (uint32_t k = 0; k < n_profiles; ++k)
        if (st[k] != MSV_OK) return st[k];
    return MSV_OK;
}

msv_status msv_score_fasta_device(msv_profile* p, const msv_fasta_device* fasta, float* scores) {
    if (!p || !fasta) return MSV_ERR_INVALID_ARGUMENT;
    if (msv_fasta_device_device(fasta) != p->device) return MSV_ERR_INVALID_ARGUMENT;  // another GPU's memory
    const uint64_t n = msv_fasta_device_count(fasta);
    if (n == 0) return MSV_OK;
    if (!scores) return MSV_ERR_INVALID_ARGUMENT;
    msv_status s = msv_profile_reserve_length(p, msv_fasta_device_max_length(fasta));
    if (s != MSV_OK) return s;
    DeviceGuard g(p->device);
    if (!g.ok) return MSV_ERR_NO_DEVICE;
    CsrStaging& sg = p->host;  // (only its order and scores: the inputs are the parser's)
    MSV_HIP(sg.reserve_results(n, n));
    const uint64_t* d_off = msv_fasta_device_offsets(fasta);
    s = msv_order_longest_first(p, d_off, n, sg.d_order, p->stream);
    if (s != MSV_OK) return s;
    s = msv_score_batch_device(p, msv_fasta_device_codes(fasta), std::max<uint64_t>(msv_fasta_device_residues(fasta), 1),
                               d_off, n, sg.d_order, sg.d_scores, p->stream);
    if (s != MSV_OK) return s;
    MSV_HIP(hipMemcpyAsync(scores, sg.d_scores, n * sizeof(float), hipMemcpyDeviceToHost, p->stream));
    return msv_profile_check(p, p->stream);
}

}  // extern "C"
