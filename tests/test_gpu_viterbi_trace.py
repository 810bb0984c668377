"""The Viterbi trace on the GPU (Viterbi_HMM.trace_batch, vit_trace.hip) against the CPU trace
(msv_vit_cpu_trace, itself pinned by tests/test_viterbi_trace_host.py): score bits, domains and ops are EQUAL,
not merely equally good -- both derive every source by equality on final values in one tie-break order.  The
scores also equal Viterbi_HMM.score_batch's, bitwise."""
import ctypes as C

import numpy as np
import pytest

import hmm_fasta_viterbi_amd as msv
from hmm_fasta_viterbi_amd import _native
from hmm_fasta_viterbi_amd.synthetic import (concat_batches, gapped_homolog_batch, homolog_batch, random_batch,
                                             write_hmm)
from oracle_lib import bits, profile_path
from state_batches import _csr, boundary_batch, edge_batch, tail_gapped_batch
from test_viterbi_trace_host import host_tables, stress_tables, tiny_cases
from trace_check import F, assert_same, cpu_traces, profile_from_tables, tables_of, traces_lists, two_core_batch

pytestmark = pytest.mark.gpu

PLANS = msv.Viterbi_HMM.trace_plans()


def check(vit, codes, offsets, what="", **kw):
    """trace_batch of the whole batch == the CPU trace; scores == score_batch.  Returns the Traces."""
    t = vit.trace_batch(codes=codes, offsets=offsets, **kw)
    assert_same(t, cpu_traces(tables_of(vit), codes, offsets), what)
    assert np.array_equal(bits(t.scores), bits(vit.score_batch(codes=codes, offsets=offsets))), what
    return t


def test_tiny_models():
    """LENG 1..5, inserts off and on, distinct exits, L 0..5, through msv_vit_profile_create on tables."""
    for msc, isc, tsc, consts, seqs in tiny_cases():
        vit = profile_from_tables(msc, isc, tsc, consts)
        try:
            check(vit, *_csr(seqs), what=(msc.shape[1] - 1, isc is not None))
        finally:
            vit.close()


def exact_fit_lengths():
    out, prev = [1, 2, 3], 0
    for _, cap in PLANS:
        out += [prev + 1, cap - 1, cap]
        prev = cap
    return sorted(set(out))


_models = {}


def synthetic(leng, tmp_path_factory):
    if leng not in _models:
        path = str(tmp_path_factory.mktemp("trace_hmm") / f"{leng}.hmm")
        write_hmm(path, leng, 500 + leng)
        _models[leng] = msv.Profile_HMM(path)
    return _models[leng]


def lengths_batch(seed, lengths):
    rng = np.random.Generator(np.random.PCG64(seed))
    return _csr([rng.integers(0, 20, size=L, dtype=np.uint8) for L in lengths])


@pytest.mark.parametrize("leng", exact_fit_lengths())
def test_exact_fit_lengths(leng, tmp_path_factory):
    """Every plan at its capacity, capacity - 1 and the previous plan's capacity + 1, and LENG 1, 2, 3: windows
    across lane, word and wave boundaries and the last states, paths that end in the last nodes, and the edge
    lengths around the 64-row residue block (0, 1, 2, 63, 64, 65, 128, 129)."""
    hmm = synthetic(leng, tmp_path_factory)
    vit = msv.Viterbi_HMM(hmm)
    info = vit.trace_describe()
    assert info["capacity"] >= leng and info["scratch_bytes"] == 0
    assert info["plan"] == [name for name, cap in PLANS if cap >= leng][0]
    S = info["states_per_lane"]
    bounds = [S, 8, 64 * S, leng - 1, leng - S, info["capacity"] // 2]
    (bc, bo), _ = boundary_batch(hmm.match_emissions, leng, bounds, viterbi=True)
    keep = np.arange(0, len(bo) - 1, 5)   # ~15 of its sequences, every kind among them
    picked = _csr([bc[int(bo[i]):int(bo[i + 1])] for i in keep])
    batch = concat_batches(picked, tail_gapped_batch(hmm.match_emissions, leng + 2, 4, 8, 130), edge_batch(leng + 3),
                           lengths_batch(leng + 4, (128, 129)))
    t = check(vit, *batch, what=leng)
    assert len(t) >= 20


@pytest.mark.parametrize("prof", ["100.hmm", "1400.hmm", "2405.hmm"])
def test_lazy_f_stress(prof):
    """d->d 0.995, m->d 0.3, d->m 0.9: long D chains, so D pointers cross lane, word and wave boundaries."""
    hmm, tables = host_tables(prof)
    vit = profile_from_tables(*stress_tables(tables))
    try:
        batch = concat_batches(gapped_homolog_batch(hmm.match_emissions, 31, 8, 40, 300),
                               tail_gapped_batch(hmm.match_emissions, 32, 4, 8, 130), edge_batch(33))
        t = check(vit, *batch, what=prof)
        ops = t.ops.tobytes()
        assert b"D" * 9 in ops  # chains longer than a lane's 8 states
    finally:
        vit.close()


def test_distinct_exit_constants():
    """tr_E_C != tr_E_J: the C flags then differ from the J flags; two planted cores give two domains."""
    hmm, (msc, isc, tsc, (b, c, j)) = host_tables("1400.hmm")
    vit = profile_from_tables(msc, isc, tsc, (b, F(F(c) - F(0.75)), j))
    try:
        batch = concat_batches(two_core_batch(hmm.match_emissions, 3, 8), homolog_batch(hmm.match_emissions, 4, 6, 1, 200),
                               edge_batch(5))
        t = check(vit, *batch)
        assert max(len(d) for d in traces_lists(t)) >= 2
    finally:
        vit.close()


@pytest.mark.parametrize("prof", ["100.hmm", "1400.hmm"])
def test_informative_inserts(prof):
    hmm = msv.Profile_HMM(profile_path(prof))
    vit = msv.Viterbi_HMM(hmm, insert_mode=msv.INSERTS_LOG_ODDS)
    batch = concat_batches(gapped_homolog_batch(hmm.match_emissions, 41, 10, 30, 200), random_batch(42, 4, 1, 130),
                           edge_batch(43))
    check(vit, *batch, what=prof)


def test_queue_depth():
    """3 x the launch's resident sequence slots + 1 short sequences on a tiny model: every workgroup dequeues
    three rounds deep."""
    rng = np.random.Generator(np.random.PCG64(77))
    msc, isc, tsc, consts = next(c for c in tiny_cases() if c[0].shape[1] == 4)[:4]
    vit = profile_from_tables(msc, isc, tsc, consts)
    try:
        slots = vit.trace_describe()["blocks"]
        n = 3 * slots + 1
        batch = _csr([rng.integers(0, 20, size=int(L), dtype=np.uint8) for L in rng.integers(0, 9, n)])
        t = check(vit, *batch)
        assert len(t) == n and t.stats["chunks"] == 1
    finally:
        vit.close()


def plan_index(vit):
    return [name for name, _ in PLANS].index(vit.trace_describe()["plan"])


def test_chunking():
    """A workspace that cuts the batch into >= 3 chunks, one that equals the largest sequence exactly: identical
    to the one-chunk call.  One byte less: MSV_ERR_OUT_OF_MEMORY."""
    hmm = msv.Profile_HMM(profile_path("1400.hmm"))
    vit = msv.Viterbi_HMM(hmm)
    codes, offsets = concat_batches(gapped_homolog_batch(hmm.match_emissions, 51, 10, 50, 150), edge_batch(52))
    one = check(vit, codes, offsets)
    assert one.stats["chunks"] == 1
    sizes = [int(_native.lib().msv_vit_trace_sequence_bytes(plan_index(vit), int(L))) for L in np.diff(offsets)]
    assert one.stats["pointer_bytes"] == sum(sizes)
    for workspace in (max(max(sizes), sum(sizes) // 3), max(sizes)):
        t = vit.trace_batch(codes=codes, offsets=offsets, workspace_bytes=workspace)
        assert t.stats["chunks"] >= 3 and t.stats["pointer_bytes"] == sum(sizes)
        assert np.array_equal(bits(t.scores), bits(one.scores))
        assert np.array_equal(t.domain_offsets, one.domain_offsets)
        assert np.array_equal(t.domains, one.domains) and np.array_equal(t.ops, one.ops)
    with pytest.raises(msv.MSVError) as e:
        vit.trace_batch(codes=codes, offsets=offsets, workspace_bytes=max(sizes) - 1)
    assert e.value.name == "MSV_ERR_OUT_OF_MEMORY"
    check(vit, codes, offsets)  # the refusal left the profile usable


def test_select_lists():
    hmm = msv.Profile_HMM(profile_path("400.hmm"))
    vit = msv.Viterbi_HMM(hmm)
    codes, offsets = concat_batches(homolog_batch(hmm.match_emissions, 61, 12, 1, 150), edge_batch(62))
    n = len(offsets) - 1
    want = cpu_traces(tables_of(vit), codes, offsets)
    rng = np.random.Generator(np.random.PCG64(63))
    shuffled = rng.permutation(n).astype(np.uint32)
    repeated = np.array([3, 3, 0, n - 1, 3, 7, 0], np.uint32)
    for sel in (shuffled, repeated, shuffled[:5]):
        t = vit.trace_batch(codes=codes, offsets=offsets, select=sel)
        assert_same(t, [want[int(s)] for s in sel], sel)
        assert [int(d["seq"]) for q in range(len(t)) for d in t.domains_of(q)] == \
               [int(s) for s in sel for _ in want[int(s)][1]]
    empty = vit.trace_batch(codes=codes, offsets=offsets, select=np.zeros(0, np.uint32))
    assert len(empty) == 0 and len(empty.domains) == 0 and len(empty.ops) == 0 and list(empty.domain_offsets) == [0]
    with pytest.raises(msv.MSVError) as e:
        vit.trace_batch(codes=codes, offsets=offsets, select=np.array([0, n], np.uint32))
    assert e.value.name == "MSV_ERR_INVALID_ARGUMENT"


def test_bad_input_in_a_batch():
    """A bad residue: the scoring call's status, that entry +inf and without domains, the others traced.  A
    sequence too long for any length table: the scoring call's refusal of the whole call."""
    hmm = msv.Profile_HMM(profile_path("400.hmm"))
    vit = msv.Viterbi_HMM(hmm)
    codes, offsets = homolog_batch(hmm.match_emissions, 71, 9, 20, 150)
    want = cpu_traces(tables_of(vit), codes, offsets)
    bad = codes.copy()
    bad[int(offsets[4]) + 3] = 22
    with pytest.raises(IndexError):
        vit.score_batch(codes=bad, offsets=offsets)
    with pytest.raises(IndexError):
        vit.trace_batch(codes=bad, offsets=offsets)
    t = vit.trace_batch(codes=bad, offsets=offsets, strict=False)
    assert t.status == "MSV_ERR_BAD_RESIDUE"
    assert np.isposinf(t.scores[4]) and len(t.domains_of(4)) == 0
    got = traces_lists(t)
    for q in range(len(want)):
        if q != 4:
            assert bits(t.scores[q]) == bits(want[q][0]) and got[q] == want[q][1]
    check(vit, codes, offsets)  # the error word was cleared
    # offsets that claim a sequence of 2^31 residues are refused before any residue is read
    long_off = np.array([0, 5, 5 + 2 ** 31], np.uint64)
    out = np.zeros(2, np.float32)
    L = _native.lib()
    st = L.msv_vit_score_batch(vit._p, codes.ctypes.data, long_off.ctypes.data, 2, out.ctypes.data, None)
    p = C.c_void_p()
    assert L.msv_vit_trace_batch(vit._p, codes.ctypes.data, long_off.ctypes.data, 2, None, 0, 0, C.byref(p)) == st
    assert _native.STATUS[st] == "MSV_ERR_SEQUENCE_TOO_LONG" and not p.value


def test_filter_pipeline_align():
    """filter_pipeline(align=True) == filter_pipeline + trace_batch on the passed indices, 1400.hmm x a
    300-sequence mixed batch."""
    hmm = msv.Profile_HMM(profile_path("1400.hmm"))
    eng, vit = msv.MSV_HMM(hmm), msv.Viterbi_HMM(hmm)
    me = hmm.match_emissions
    codes, offsets = concat_batches(random_batch(81, 200, 30, 400), homolog_batch(me, 82, 60, 30, 400),
                                    gapped_homolog_batch(me, 83, 40, 30, 400))
    msc, mask, vsc, vpv, traces = msv.filter_pipeline(eng, vit, codes=codes, offsets=offsets, align=True)
    plain = msv.filter_pipeline(eng, vit, codes=codes, offsets=offsets)
    assert len(plain) == 4 and np.array_equal(plain[1], mask) and np.array_equal(bits(plain[2]), bits(vsc))
    passed = np.flatnonzero(mask)
    assert 50 <= len(passed) < 300 and len(traces) == len(passed)
    manual = vit.trace_batch(codes=codes, offsets=offsets, select=passed.astype(np.uint32))
    assert np.array_equal(bits(traces.scores), bits(manual.scores)) and np.array_equal(traces.ops, manual.ops)
    assert np.array_equal(traces.domains, manual.domains)
    assert np.array_equal(bits(traces.scores), bits(vsc[passed]))
    assert_same(traces, cpu_traces(tables_of(vit), codes, offsets, passed))
    # the reading aids agree with the domains
    q = int(np.argmax([len(traces.domains_of(q)) for q in range(len(traces))]))
    path = list(traces.path(q))
    d0 = traces.domains_of(q)[0]
    assert path[0] == ("M", int(d0["k_from"]), int(d0["i_from"])) and len(path) == int(traces.domains_of(q)["ops_len"].sum())
    lines = traces.alignment(q, 0).split("\n")
    assert len(lines) == 3 and len(lines[0]) == len(lines[1]) == len(lines[2]) == int(d0["ops_len"])
