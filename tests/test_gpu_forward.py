"""GPU parity of the Forward stage (fwd_kernel.hip through the C-ABI) against the library's float64 CPU
Forward (msv_fwd_cpu_score, itself pinned on the CPU by test_forward_paths.py and test_forward_host.py).

Tolerance, derived in DESIGN 4.9 and stated in msv.h, never tuned: every term of the recurrence is non-negative, so
nothing cancels and the relative error of the summed odds is at most the roundings along the deepest path (L + LENG
state steps, under 16 roundings each) times 2^-24, plus the float output's own rounding:
    |gpu - cpu64| <= 16 (L + LENG) 2^-24 + 4 2^-24 |cpu64|  nats,   -inf / +inf / NaN classes equal.
The bound is loose, so the models used here are ones in which every term of the model moves the score by far more
than it (shown on the CPU in test_forward_host.py): the stress transitions for the D chain, the D -> E exits and
d->m, log-odds inserts on gapped homologs for the I states, repeated homologs for the J loop.
Measured on the GPU (assert_close prints it): DESIGN 4.9 records the worst error per test."""
import json
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import hmm_fasta_viterbi_amd as msv
from hmm_fasta_viterbi_amd import _native
from hmm_fasta_viterbi_amd.synthetic import (background_batch, concat_batches, gapped_homolog_batch, homolog_batch,
                                             random_batch, write_hmm)
from forward_lib import (assert_close, cpu_scores, create_profile, destroy_profile, distinct_exits, gpu_scores,
                         stress_transitions, tables)
from oracle_lib import PROFILES, ROOT, bits, profile_path
from queue_batches import take_sequences

_hmm = {}
_fwd = {}


def hmm(prof):
    if prof not in _hmm:
        _hmm[prof] = msv.Profile_HMM(profile_path(prof))
    return _hmm[prof]


def fwd(prof, insert_mode=0) -> msv.Forward_HMM:
    key = (prof, insert_mode)
    if key not in _fwd:
        _fwd[key] = msv.Forward_HMM(hmm(prof), insert_mode=insert_mode)
    return _fwd[key]


def edge_lengths_batch(seed):
    edge = np.array([0, 1, 2, 63, 64, 65, 127, 128, 129], np.uint64)
    rng = np.random.Generator(np.random.PCG64(seed))
    codes = rng.integers(0, 20, int(edge.sum()), dtype=np.uint8)
    offsets = np.zeros(len(edge) + 1, np.uint64)
    np.cumsum(edge, out=offsets[1:])
    return codes, offsets


def mixed_batch(me, seed, n_each, lmin, lmax):
    return concat_batches(random_batch(seed, n_each, lmin, lmax), homolog_batch(me, seed + 1, n_each, lmin, lmax),
                          gapped_homolog_batch(me, seed + 2, n_each, lmin, lmax))


def repeated_homologs(me, seed, copies):
    """`copies` different homologs of 100 residues each, concatenated into ONE sequence (a multi-hit target)."""
    codes, _ = homolog_batch(me, seed, copies, 100, 100, mutate=0.0)
    return codes, np.array([0, 100 * copies], np.uint64)


def device_batch(codes, offsets):
    import torch
    dev = torch.device("cuda:0")
    return torch.from_numpy(codes).to(dev), torch.from_numpy(offsets.view(np.int64)).to(dev)


# ---- every variant at exact fit -----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", msv.Forward_HMM.variants())
def test_every_variant_at_exact_fit(name, tmp_path):
    """Every compiled variant on synthetic models of LENG 64 S and 64 S - 1 (no padding state / one), the smallest S
    also on LENG 1, 2, 3 and 65: edge lengths, background, homologs and gapped homologs, about 40 sequences."""
    S = int(re.match(r"fwd_s(\d+)", name).group(1))
    mode = 1 if name.endswith("i") else 0
    lengs = [64 * S, 64 * S - 1] + ([1, 2, 3, 65] if S == 2 else [])
    for leng in lengs:
        path = str(tmp_path / f"{leng}.hmm")
        write_hmm(path, leng, 900 + leng)
        h = msv.Profile_HMM(path)
        msc, isc, tsc, consts = tables(h, mode)
        codes, offsets = concat_batches(edge_lengths_batch(leng), mixed_batch(h.match_emissions, 40 + leng, 10, 1, 300))
        want = cpu_scores(msc, isc, tsc, consts, codes, offsets)
        p = create_profile(msc, isc, tsc, consts, name)
        try:
            info = _native.FwdInfo()
            assert _native.lib().msv_fwd_profile_describe(p, info) == 0
            assert info.variant.decode() == name and info.states_per_lane == S and info.scratch_bytes == 0, info.as_dict()
            st, got = gpu_scores(p, codes, offsets)
            assert st == 0
            assert_close(got, want, offsets, leng, f"{name} LENG {leng}")
        finally:
            destroy_profile(p)


def test_model_beyond_the_family_is_unsupported():
    M = 2434  # LENG 2433
    msc = np.zeros((20, M), np.float32)
    tsc = np.full((M, 7), np.float32(np.log(0.5)), np.float32)
    import ctypes as C
    p = C.c_void_p()
    assert _native.lib().msv_fwd_profile_create(0, msc.ctypes.data, None, tsc.ctypes.data, M, -8.0, -0.69, -0.69,
                                                C.byref(p)) == 6  # MSV_ERR_UNSUPPORTED_MODEL
    e = fwd("100.hmm")
    with pytest.raises(msv.MSVError):
        msv.Forward_HMM(hmm("300.hmm")).set_variant("fwd_s2")  # 128 states do not hold LENG 300
    with pytest.raises(msv.MSVError):
        e.set_variant("fwd_s2i")  # an insert-odds variant on a profile without them


# ---- rescaling ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("prof,mode", [("100.hmm", 0), ("300.hmm", 1)])
def test_rescaling_on_concatenated_homologs(prof, mode):
    """Scores far beyond float32's 88.7 nats of odds: ten sequences of 20 .. 38 concatenated homologs and one of 80,
    whose running E passes the 2^32 threshold (22 nats) dozens of times."""
    me = hmm(prof).match_emissions
    batch = concat_batches(*[repeated_homologs(me, 70 + c, c) for c in list(range(20, 40, 2)) + [80]],
                           random_batch(5, 3, 200, 900))
    codes, offsets = batch
    e = fwd(prof, mode)
    want = e.cpu_score_batch(codes=codes, offsets=offsets)
    assert np.sum(want > 100.0) >= 8, want
    assert want.max() > 5 * 22.2, want  # several crossings of 2^32 in one sequence
    got = e.score_batch(codes=codes, offsets=offsets)
    assert_close(got, want, offsets, hmm(prof).model_length - 1, f"rescaling {prof}")


# ---- the D-scan stress model -----------------------------------------------------------------------------------

@pytest.mark.parametrize("prof,variant", [("1400.hmm", None), ("1400.hmm", "fwd_s38g4"), ("2405.hmm", None)])
def test_d_scan_stress_model(prof, variant):
    """d->d 0.995, m->d 0.9, d->m 0.3 (test_gpu_viterbi.py's stress transitions) and distinct exits on 1,400 and 2,405
    states: D mass crosses many lanes in every row, so the scan, its constants and the D -> E exits carry the score."""
    msc, isc, tsc, consts = tables(hmm(prof), 0)
    tsc, consts = stress_transitions(tsc), distinct_exits(consts)
    codes, offsets = concat_batches(edge_lengths_batch(3), mixed_batch(hmm(prof).match_emissions, 61, 10, 1, 300))
    want = cpu_scores(msc, None, tsc, consts, codes, offsets)
    p = create_profile(msc, None, tsc, consts, variant)
    try:
        st, got = gpu_scores(p, codes, offsets)
        assert st == 0
        assert_close(got, want, offsets, msc.shape[1] - 1, f"stress {prof} {variant}")
    finally:
        destroy_profile(p)


# ---- queue depth ------------------------------------------------------------------------------------------------

def test_every_wave_scores_several_sequences_in_a_row():
    """2 x (blocks x waves_per_block) + 3 short sequences, homologs and background mixed and shuffled: every wave
    takes several sequences, so a scale exponent, N, J or C that survived from the previous sequence shows."""
    prof = "100.hmm"
    e = fwd(prof)
    info = e.describe()
    n = 2 * info["blocks"] * info["waves_per_block"] + 3
    me = hmm(prof).match_emissions
    k = n // 3
    codes, offsets = concat_batches(homolog_batch(me, 81, k, 1, 130), random_batch(82, n - 2 * k, 0, 130),
                                    gapped_homolog_batch(me, 83, k, 1, 130))
    codes, offsets = take_sequences(codes, offsets, np.random.Generator(np.random.PCG64(84)).permutation(n))
    want = e.cpu_score_batch(codes=codes, offsets=offsets)
    got = e.score_batch(codes=codes, offsets=offsets)
    assert_close(got, want, offsets, 100, f"queue depth n = {n}")


def test_long_and_short_sequences_alternate_on_one_wave():
    """A rescaled sequence (exponent far from 0) followed by short ones on the same waves: one workgroup's worth of
    waves, four times as many sequences."""
    prof = "100.hmm"
    e = fwd(prof)
    me = hmm(prof).match_emissions
    long_ones = [repeated_homologs(me, 90 + c, 12) for c in range(8)]
    short = [random_batch(100 + c, 3, 1, 40) for c in range(8)]
    codes, offsets = concat_batches(*[b for pair in zip(long_ones, short) for b in pair])
    want = e.cpu_score_batch(codes=codes, offsets=offsets)
    got = e.score_batch(codes=codes, offsets=offsets)
    assert_close(got, want, offsets, 100, "long / short alternation")


# ---- determinism ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("prof", ["300.hmm", "1400.hmm"])
def test_scores_do_not_depend_on_position_or_run(prof):
    e = fwd(prof)
    codes, offsets = mixed_batch(hmm(prof).match_emissions, 111, 60, 1, 400)
    n = len(offsets) - 1
    a = e.score_batch(codes=codes, offsets=offsets)
    b = e.score_batch(codes=codes, offsets=offsets)
    assert np.array_equal(bits(a), bits(b))
    perm = np.random.Generator(np.random.PCG64(112)).permutation(n)
    pc, po = take_sequences(codes, offsets, perm)
    c = e.score_batch(codes=pc, offsets=po)
    assert np.array_equal(bits(c), bits(a[perm]))


def test_select_list_and_device_count():
    """A device select list with its count in device memory scores exactly the listed sequences, each at its own
    index, with the bits of a whole-batch launch; the others are untouched."""
    import torch
    prof = "1400.hmm"
    e = fwd(prof)
    codes, offsets = mixed_batch(hmm(prof).match_emissions, 121, 40, 50, 400)
    n = len(offsets) - 1
    whole = e.score_batch(codes=codes, offsets=offsets)
    d_res, d_off = device_batch(codes, offsets)
    sel = np.arange(0, n, 3, dtype=np.uint32)[::-1].copy()
    d_sel = torch.from_numpy(sel.view(np.int32)).to(d_res.device)
    d_cnt = torch.tensor([len(sel)], dtype=torch.int32, device=d_res.device)
    d_sc = torch.full((n,), 7.0, dtype=torch.float32, device=d_res.device)
    st = torch.cuda.Stream(d_res.device)
    torch.cuda.synchronize()
    e.score_batch_device(d_res.data_ptr(), codes.size, d_off.data_ptr(), n, d_sc.data_ptr(), d_sel.data_ptr(),
                         d_cnt.data_ptr(), st.cuda_stream)
    st.synchronize()
    e.check(st.cuda_stream)
    got = d_sc.cpu().numpy()
    mask = np.zeros(n, bool)
    mask[sel] = True
    assert np.array_equal(bits(got[mask]), bits(whole[mask]))
    assert np.all(got[~mask] == 7.0)


def test_select_count_beyond_the_batch_is_clamped_and_latched():
    import torch
    prof = "300.hmm"
    e = fwd(prof)
    codes, offsets = random_batch(98, 40, 20, 300)
    n = len(offsets) - 1
    whole = e.score_batch(codes=codes, offsets=offsets)
    d_res, d_off = device_batch(codes, offsets)
    # the list's n entries, then 64 more valid ones: only the count check can report them
    sel = np.concatenate([np.arange(n, dtype=np.uint32)[::-1], np.zeros(64, np.uint32)])
    d_sel = torch.from_numpy(sel.view(np.int32)).to(d_res.device)
    d_cnt = torch.tensor([n + 64], dtype=torch.int32, device=d_res.device)
    d_sc = torch.full((n,), 7.0, dtype=torch.float32, device=d_res.device)
    st = torch.cuda.Stream(d_res.device)
    torch.cuda.synchronize()
    e.score_batch_device(d_res.data_ptr(), codes.size, d_off.data_ptr(), n, d_sc.data_ptr(), d_sel.data_ptr(),
                         d_cnt.data_ptr(), st.cuda_stream)
    with pytest.raises(msv.MSVError):
        e.check(st.cuda_stream)
    e.check(st.cuda_stream)  # reported once, then cleared
    assert np.array_equal(bits(d_sc.cpu().numpy()), bits(whole))
    # a list entry outside the batch is reported and skipped
    sel = np.array([3, n + 5, 7, 0xFFFFFFFF, 11], np.uint32)
    d_sel = torch.from_numpy(sel.view(np.int32)).to(d_res.device)
    d_cnt = torch.tensor([len(sel)], dtype=torch.int32, device=d_res.device)
    d_sc.fill_(7.0)
    torch.cuda.synchronize()
    e.score_batch_device(d_res.data_ptr(), codes.size, d_off.data_ptr(), n, d_sc.data_ptr(), d_sel.data_ptr(),
                         d_cnt.data_ptr(), st.cuda_stream)
    with pytest.raises(msv.MSVError):
        e.check(st.cuda_stream)
    got = d_sc.cpu().numpy()
    assert np.array_equal(bits(got[[3, 7, 11]]), bits(whole[[3, 7, 11]]))
    assert np.all(np.delete(got, [3, 7, 11]) == 7.0)


# ---- errors and streams ------------------------------------------------------------------------------------------

def test_empty_bad_residue_and_too_long():
    import torch
    e = msv.Forward_HMM(hmm("200.hmm"))
    try:
        codes, offsets = random_batch(3, 6, 0, 50)
        lens = np.diff(offsets.astype(np.int64))
        got = e.score_batch(codes=codes, offsets=offsets)
        assert np.all(np.isneginf(got[lens == 0])) and np.all(np.isfinite(got[lens > 0]))
        bad = codes.copy()
        first = int(np.flatnonzero(lens > 0)[0])
        bad[int(offsets[first])] = 20
        with pytest.raises(IndexError):
            e.score_batch(codes=bad, offsets=offsets)
        e.check()  # the host call reported and cleared its own error
        assert np.array_equal(bits(e.score_batch(codes=codes, offsets=offsets)), bits(got))
        # the device path: +inf at the bad sequence, the others scored; NaN beyond the reserved length
        d_res, d_off = device_batch(bad, offsets)
        n = len(lens)
        d_sc = torch.full((n,), 7.0, dtype=torch.float32, device=d_res.device)
        st = torch.cuda.Stream(d_res.device)
        torch.cuda.synchronize()
        e.score_batch_device(d_res.data_ptr(), bad.size, d_off.data_ptr(), n, d_sc.data_ptr(), stream=st.cuda_stream)
        with pytest.raises(IndexError):
            e.check(st.cuda_stream)
        dev = d_sc.cpu().numpy()
        assert dev[first] == np.inf
        others = np.arange(n) != first
        assert np.array_equal(bits(dev[others]), bits(got[others]))
        max_len = e.describe()["max_length"]
        L = max_len + 1
        long_codes = np.zeros(L + 10, np.uint8)
        long_off = np.array([0, 10, 10 + L], np.uint64)
        d_res, d_off = device_batch(long_codes, long_off)
        d_sc = torch.full((2,), 7.0, dtype=torch.float32, device=d_res.device)
        torch.cuda.synchronize()
        e.score_batch_device(d_res.data_ptr(), long_codes.size, d_off.data_ptr(), 2, d_sc.data_ptr(),
                             stream=st.cuda_stream)
        with pytest.raises(msv.MSVError) as err:
            e.check(st.cuda_stream)
        assert err.value.name == "MSV_ERR_SEQUENCE_TOO_LONG"
        dev = d_sc.cpu().numpy()
        assert np.isnan(dev[1]) and np.isfinite(dev[0])
    finally:
        e.close()


def test_one_profile_on_two_streams_without_sync():
    """Launches of one Forward profile on two caller streams plus the synchronous host call on the library's stream,
    no synchronisation between them: each takes its own dequeue-counter slot.  Bitwise against a lone launch."""
    import torch
    prof = "1400.hmm"
    e = fwd(prof)
    me = hmm(prof).match_emissions
    batches = [concat_batches(random_batch(500 + k, n, 50, 400), homolog_batch(me, 600 + k, n // 10, 50, 400))
               for k, n in enumerate((1500, 400, 1200))]
    ref = [e.score_batch(codes=c, offsets=off) for c, off in batches]
    want = e.cpu_score_batch(codes=batches[1][0], offsets=batches[1][1])
    assert_close(ref[1], want, batches[1][1], 1400, "two streams, reference batch")
    streams = [torch.cuda.Stream(torch.device("cuda:0")) for _ in range(2)]
    tens = [device_batch(c, off) for c, off in batches]
    for rep in range(3):
        outs = {k: torch.full((len(batches[k][1]) - 1,), float("nan"), dtype=torch.float32, device="cuda:0")
                for k in (0, 2)}
        torch.cuda.synchronize()
        r, off = tens[0]
        e.score_batch_device(r.data_ptr(), r.numel(), off.data_ptr(), outs[0].numel(), outs[0].data_ptr(),
                             stream=streams[0].cuda_stream)
        host = e.score_batch(codes=batches[1][0], offsets=batches[1][1])  # library stream, no sync first
        r, off = tens[2]
        e.score_batch_device(r.data_ptr(), r.numel(), off.data_ptr(), outs[2].numel(), outs[2].data_ptr(),
                             stream=streams[1].cuda_stream)
        torch.cuda.synchronize()
        e.check()
        assert np.array_equal(bits(host), bits(ref[1])), rep
        for k in (0, 2):
            assert np.array_equal(bits(outs[k].cpu().numpy()), bits(ref[k])), (rep, k)
        e.bind_stream(streams[0].cuda_stream if rep == 0 else None)


def test_residue_offsets_beyond_2_to_32():
    """The kernel forms residue addresses from 64-bit offsets made wave-uniform half by half: a device batch that
    straddles byte 2^32 of one buffer scores exactly as at offset 0."""
    import torch
    prof = "300.hmm"
    e = fwd(prof)
    codes, offsets = mixed_batch(hmm(prof).match_emissions, 131, 20, 1, 130)
    n, total = len(offsets) - 1, int(offsets[-1])
    whole = e.score_batch(codes=codes, offsets=offsets)
    size = (1 << 32) + (1 << 16)
    base = (1 << 32) - total // 2
    buf = torch.zeros(size, dtype=torch.uint8, device="cuda:0")
    try:
        buf[base:base + total] = torch.from_numpy(codes).to(buf.device)
        off = offsets.astype(np.uint64) + np.uint64(base)
        assert off[0] < (1 << 32) <= off[n // 2] and off[-1] > (1 << 32)
        d_off = torch.from_numpy(off.view(np.int64)).to(buf.device)
        d_sc = torch.full((n,), 7.0, dtype=torch.float32, device=buf.device)
        st = torch.cuda.Stream(buf.device)
        torch.cuda.synchronize()
        e.score_batch_device(buf.data_ptr(), size, d_off.data_ptr(), n, d_sc.data_ptr(), stream=st.cuda_stream)
        st.synchronize()
        e.check(st.cuda_stream)
        assert np.array_equal(bits(d_sc.cpu().numpy()), bits(whole))
    finally:
        del buf
        torch.cuda.empty_cache()
    # the host call rebases 64-bit offsets above 2^32 (a lazily allocated zero buffer)
    hbase = (1 << 32) + 123457
    host = np.zeros(hbase + total, np.uint8)
    host[hbase:] = codes
    assert np.array_equal(bits(e.score_batch(codes=host, offsets=offsets.astype(np.uint64) + np.uint64(hbase))),
                          bits(whole))


# ---- all bundled profiles -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("prof", PROFILES)
def test_every_bundled_profile(prof):
    e = fwd(prof)
    fa = msv.FASTA_protein_sequences(os.path.join(ROOT, "data", "FASTA_files", "fasta_like_example.fsa"))
    codes, offsets = concat_batches((fa.codes, fa.offsets), random_batch(int(prof.split(".")[0]), 24, 1, 600))
    want = e.cpu_score_batch(codes=codes, offsets=offsets)
    got = e.score_batch(codes=codes, offsets=offsets)
    assert_close(got, want, offsets, hmm(prof).model_length - 1, prof)
    s = fa.sequences[3]
    assert abs(e.parallel_run_on_sequence(s) - e.run_on_sequence(s)) <= 1e-3


# ---- the cascade -------------------------------------------------------------------------------------------------

def test_search_pipeline_equals_the_stages_composed_by_hand():
    """search_pipeline = score_batch / pvalues / masks of the three engines composed on the host: bitwise on the
    scores, exact on the masks.  1400.hmm, 2,000 background sequences plus 50 homologs."""
    prof = "1400.hmm"
    h = hmm(prof)
    m, v, f = msv.MSV_HMM(h), msv.Viterbi_HMM(h), fwd(prof)
    try:
        codes, offsets = concat_batches(random_batch(141, 2000, 100, 500), homolog_batch(h.match_emissions, 142, 50, 200, 600))
        n = len(offsets) - 1
        perm = np.random.Generator(np.random.PCG64(143)).permutation(n)
        codes, offsets = take_sequences(codes, offsets, perm)
        r = msv.search_pipeline(m, v, f, codes=codes, offsets=offsets)
        msc = m.score_batch(codes=codes, offsets=offsets)
        assert np.array_equal(bits(r["msv_scores"]), bits(msc))
        p1 = m.pvalues(msc, offsets) <= 0.02
        assert np.array_equal(r["passed_msv"], p1) and 0 < p1.sum() < n
        vsc = v.score_batch(codes=codes, offsets=offsets)
        assert np.array_equal(bits(r["vit_scores"][p1]), bits(vsc[p1]))
        assert np.all(np.isneginf(r["vit_scores"][~p1]))
        p2 = p1 & (v.pvalues(vsc, offsets) <= 1e-3)
        assert np.array_equal(r["passed_vit"], p2) and 0 < p2.sum() < p1.sum()
        fsc = f.score_batch(codes=codes, offsets=offsets)
        assert np.array_equal(bits(r["fwd_scores"][p2]), bits(fsc[p2]))
        assert np.all(np.isneginf(r["fwd_scores"][~p2]))
        hand = np.where(p2, f.pvalues(fsc, offsets), 1.0)
        np.testing.assert_allclose(r["fwd_pvalues"], hand, rtol=1e-12, atol=0.0)  # (device exp vs host exp)
        assert np.all(r["fwd_pvalues"][~p2] == 1.0)
        print(f"cascade: {n} sequences, {p1.sum()} pass MSV, {p2.sum()} pass Viterbi, "
              f"{int(np.sum(r['fwd_pvalues'] < 1e-3))} with Forward P < 1e-3")
        # other thresholds, and an empty batch
        r2 = msv.search_pipeline(m, v, f, codes=codes, offsets=offsets, F1=1.0, F2=0.5)
        assert r2["passed_msv"].all() and np.array_equal(r2["passed_vit"], v.pvalues(vsc, offsets) <= 0.5)
        assert np.array_equal(bits(r2["fwd_scores"][r2["passed_vit"]]), bits(fsc[r2["passed_vit"]]))
        r0 = msv.search_pipeline(m, v, f, codes=np.zeros(0, np.uint8), offsets=np.zeros(1, np.uint64))
        assert len(r0["fwd_scores"]) == 0
    finally:
        m.close()
        v.close()


def test_device_pvalues_equal_the_host_formula():
    import torch
    prof = "500.hmm"
    e = fwd(prof)
    codes, offsets = mixed_batch(hmm(prof).match_emissions, 151, 50, 0, 300)
    n = len(offsets) - 1
    sc = e.score_batch(codes=codes, offsets=offsets)
    want = e.pvalues(sc, offsets)
    d_sc = torch.from_numpy(sc).to("cuda:0")
    _, d_off = device_batch(codes, offsets)
    d_pv = torch.zeros(n, dtype=torch.float64, device="cuda:0")
    st = torch.cuda.Stream(torch.device("cuda:0"))
    torch.cuda.synchronize()
    e.pvalues_device(d_sc.data_ptr(), d_off.data_ptr(), n, d_pv.data_ptr(), st.cuda_stream)
    st.synchronize()
    np.testing.assert_allclose(d_pv.cpu().numpy(), want, rtol=1e-12, atol=0.0)


# ---- calibration ---------------------------------------------------------------------------------------------

def calibration_record():
    path = os.path.join(ROOT, "profiles", "fwd_calibration.jsonl")
    rows = [json.loads(line) for line in open(path)]
    return {r["profile"]: r["d_bits"] for r in rows if "profile" in r}


@pytest.mark.parametrize("prof", PROFILES)
def test_forward_tau_calibration(prof):
    """HMMER's p7_Tau sample -- 10,000 background sequences of length 100 -- scored by the kernel: d = (the empirical
    0.96-quantile of the bit scores) - tau lies within the band the float64 CPU Forward measured over all 24
    profiles (tools/fwd_calibration.py, profiles/fwd_calibration.jsonl), widened by 0.3 bits: the margin the
    Viterbi calibration test gives over its own measured range plus the quantile's sampling error, ~0.1 bit."""
    rec = calibration_record()
    lo, hi = min(rec.values()) - 0.3, max(rec.values()) + 0.3
    e = fwd(prof)
    codes, offsets = background_batch(2025, 10_000, 100)
    sc = e.score_batch(codes=codes, offsets=offsets).astype(np.float64)
    L = 100.0
    p1 = L / (L + 1.0)
    nullsc = L * np.log(p1) + np.log(1.0 - p1)
    d = float(np.quantile((sc - nullsc) / np.log(2.0), 0.96)) - e.forward_tau
    print(f"{prof}: d = {d:+.3f} bits (recorded {rec[prof]:+.3f}, band [{lo:+.3f}, {hi:+.3f}])")
    assert lo <= d <= hi, (prof, d, lo, hi)
