// seq_queue.h -- the persistent work queue of the one-sequence-per-wave stages, device side: vit_kernel.hip and
// fwd_kernel.hip whole, vit_team.hip and vit_trace.hip in part.
//
// A launch scores the entries 0 .. total-1 of a list: `select` when given (its length the device word
// `select_count`, at most n), else every sequence of the batch.  The grid is persistent: a worker (a wave, or a
// team of waves) has the entry of its own index as its first item and takes the later ones by one atomicAdd on
// counter[0], which starts at zero and hands out the grid's worker count + 0, 1, ...  counter[1] counts the
// leavers; the last one puts the pair back to zero, so the slot's next launch needs no reset (launch_ring.h).
// Refusals are latched as msvk::kErr* bits in `errors`.  `Args` is vitk::VitArgs or fwdk::FwdArgs, which name
// these fields alike; domk::DomArgs and alnk::AlnArgs do too.  (The MSV kernels' queue -- per lane group, with
// `order` -- is another one.)
#pragma once

#include <hip/hip_runtime.h>

#include "msv_kernel.h"

namespace seqq {

// A wave-uniform 64-bit value as two scalar halves.  (The builtin returns int: each half goes back to uint32_t
// before it is widened, or a low word with bit 31 set -- a residue offset in [2^31, 2^32) -- would sign-extend
// over the high word.)
__device__ __forceinline__ uint64_t u64first(uint64_t x) {
    const uint32_t hi = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<uint32_t>(x >> 32)));
    const uint32_t lo = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<uint32_t>(x)));
    return (static_cast<uint64_t>(hi) << 32) | lo;
}

// The list's length, at most n: a device count beyond the batch is latched (kErrBadOrder) and clamped, so no
// wave reads the list past its n entries.
template <class Args>
__device__ __forceinline__ uint64_t list_total(const Args& a) {
    if (!a.select_count) return a.n;
    const uint64_t c = *a.select_count;
    if (c > a.n && blockIdx.x == 0 && threadIdx.x == 0) atomicOr(a.errors, msvk::kErrBadOrder);
    return c < a.n ? c : a.n;
}

// ADD of the gridDim.x * PER_BLOCK leavers a launch counts (workgroups: PER_BLOCK = 1; waves: a workgroup's) go;
// the last to go zeroes the counter pair.  One thread calls it.
template <int PER_BLOCK, int ADD>
__device__ __forceinline__ void count_leavers(uint32_t* counter) {
    if (atomicAdd(counter + 1, static_cast<uint32_t>(ADD)) == gridDim.x * PER_BLOCK - ADD) {
        atomicExch(counter, 0u);
        atomicExch(counter + 1, 0u);
    }
}

// Entry `item` of the list: the sequence *s, its first residue *o0 and its length *L (all wave-uniform).  True
// when the sequence is to be scored; otherwise `lane` 0 refuses it here: an entry outside the batch is reported
// and never dereferenced, an empty sequence scores -inf (C_0 = -inf, as MSV_HMM.cpp:86,112), one beyond the
// length table a NaN with kErrTooLong.
template <class Args>
__device__ __forceinline__ bool take(const Args& a, uint32_t item, int lane, uint32_t* s_out, uint64_t* o0,
                                     uint64_t* L_out) {
    const uint32_t s = *s_out = __builtin_amdgcn_readfirstlane(a.select ? a.select[item] : item);
    *o0 = u64first(a.offsets[s < a.n ? s : 0]);
    const uint64_t L = *L_out = s < a.n ? u64first(a.offsets[s + 1]) - *o0 : 0;
    if (s >= a.n) {
        if (lane == 0) atomicOr(a.errors, msvk::kErrBadOrder);
    } else if (L == 0) {
        if (lane == 0) a.scores[s] = -__builtin_inff();
    } else if (L >= a.lentab_n) {
        if (lane == 0) {
            a.scores[s] = __uint_as_float(0x7fc00000u);
            atomicOr(a.errors, msvk::kErrTooLong);
        }
    } else {
        return true;
    }
    return false;
}

// The frame of a kernel whose workers are the single waves of workgroups of WAVES (`exited_s` a word of LDS, zeroed
// before a workgroup barrier; nwaves = gridDim.x * WAVES):
//     if (seqq::no_item<WAVES>(total)) { if (threadIdx.x == 0) seqq::count_leavers<1, 1>(a.counter); return; }
//     uint32_t item = blockIdx.x * WAVES + wave;
//     while (item < total) { ...; item = seqq::next_item(a.counter, lane, nwaves); }
//     seqq::last_exit<WAVES>(a.counter, &exited_s, lane);
// no_item: no entry is left for this workgroup (a device-count launch is sized for n): it leaves at once, counted like
// any other.
template <int WAVES>
__device__ __forceinline__ bool no_item(uint64_t total) {
    return static_cast<uint64_t>(blockIdx.x) * WAVES >= total;
}
__device__ __forceinline__ uint32_t next_item(uint32_t* counter, int lane, uint32_t nwaves) {
    uint32_t t = 0;
    if (lane == 0) t = atomicAdd(counter, 1u);
    return nwaves + __builtin_amdgcn_readfirstlane(t);
}
// The last workgroup to finish resets the counters for the next launch on this profile (one grid-level atomic per
// workgroup, by its last wave, counted in LDS)
template <int WAVES>
__device__ __forceinline__ void last_exit(uint32_t* counter, uint32_t* exited_s, int lane) {
    if (lane == 0) {
        __threadfence();
        if (atomicAdd(exited_s, 1u) == WAVES - 1) count_leavers<1, 1>(counter);
    }
}

}  // namespace seqq
