// host_cpu.h -- host-only internals shared by msv_hmm.cpp and the sanitizer drivers (host_common.cpp), and the
// struct_size convention of msv.h's append-only structs for every *_device.cpp and *_host.cpp.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "msv.h"

namespace msv_host {

// msv.h's append-only structs (struct_size first).  read_sized: *out is zeroed, then the caller's bytes are copied
// in, no more than either side has (null `in`: all zeros); false where the caller's struct is smaller than min_size.
template <class T>
bool read_sized(const T* in, T* out, size_t min_size) {
    std::memset(out, 0, sizeof(T));
    if (!in) return true;
    if (in->struct_size < min_size) return false;
    std::memcpy(out, in, static_cast<size_t>(std::min<uint64_t>(in->struct_size, sizeof(T))));
    return true;
}
// write_sized: no more than the caller's struct is written, and its struct_size says how much was.
template <class T>
void write_sized(T* out, T value) {
    const uint32_t size = std::min<uint32_t>(out->struct_size, static_cast<uint32_t>(sizeof(T)));
    value.struct_size = size;
    std::memcpy(out, &value, size);
}

// MSV_HMM::run_on_sequence (MSV_HMM.cpp:74-113) on codes 0..19: emission_scores is the [20][M]
// residue-major table of MSV_HMM.cpp:38-45 (M = LENG + 1), the score is C_L + tr_move.
float run_on_sequence(const float* emission_scores, size_t M, float tr_B_Mk, float tr_E_C, float tr_E_J,
                      const uint8_t* codes, size_t L);

// The Viterbi stage's DP (msv.h, msv_vit_cpu_score) on codes 0..19: msc / isc [20][M] (isc may be null:
// zero insert scores), tsc [M][7] log transitions.
float viterbi_run_on_sequence(const float* msc, const float* isc, const float* tsc, size_t M, float tr_B_Mk,
                              float tr_E_C, float tr_E_J, const uint8_t* codes, size_t L);

// The same DP with back-pointers, walked back from C(L): the score (viterbi_run_on_sequence's bits) and one
// optimal path as domains and ops (msv.h, msv_vit_cpu_trace; seq = 0, ops_begin from 0).
struct VitTrace {
    float score = 0;
    std::vector<msv_vit_domain> domains;
    std::vector<uint8_t> ops;
};
VitTrace viterbi_trace_on_sequence(const float* msc, const float* isc, const float* tsc, size_t M, float tr_B_Mk,
                                   float tr_E_C, float tr_E_J, const uint8_t* codes, size_t L);

// Kernel-layout tables (table_layout.cpp, where the layouts are written out), from the [20][model_length]
// residue-major host tables.  The device layer uploads them as they are.
// An MSV variant of G lanes per sequence, S states per lane, the first sa of them in LDS (0: the whole row).
std::vector<float> msv_variant_table(const float* es, uint32_t model_length, int G, int S, int sa);
// The lazy-E bound of a whole-row variant: [21][G] per-lane emission maxima (poison row +inf); the device
// layer appends it to the table of the variants whose kernel skips idle E maxima (msvk::lazy_e_rows).
std::vector<float> msv_lazy_bound_table(const float* es, uint32_t model_length, int G, int S);
// A cooperative MSV variant of `waves` waves of 64 lanes x S states, neighbours sharing `halo` states.
std::vector<float> msv_coop_table(const float* es, uint32_t model_length, int waves, int S, int sa, int halo);
// A Viterbi variant of S states per lane and `team` waves per sequence: match, insert (empty unless isc)
// and transition tables, each a sequence of float pairs (the kernels' float2).
struct VitTables {
    std::vector<float> et, it, tt;
};
VitTables vit_tables(const float* msc, const float* isc_tab, const float* tsc, uint32_t model_length, int S, int team,
                     bool isc);

}  // namespace msv_host
