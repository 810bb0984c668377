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
from test_viterbi_paths import lib_cpu
from test_viterbi_trace_host import host_tables, stress_tables, tiny_cases
from trace_check import (F, assert_same, cpu_trace, cpu_traces, profile_from_tables, py_trace, quantised_model, rescore,
                         tables_of, traces_lists, two_core_batch)
from trace_ties import RULES, anchored_cases, d_takes_m_before_d, e_takes_the_smallest_k, prove

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


# ---- exact ties: every tie-break rule of msv.h at the lane, word and wave edges of every plan (trace_ties) ----------

def plan_anchors(S, team, leng):
    """Slot 0 of a lane in mid-wave (its left neighbour's values come through LDS), a lane's last slot, the second
    pointer word of a 16-state lane, and for a team the last state of wave 0 and the first of waves 1 and 3."""
    out = [S + 1, 2 * S]
    if S > 8:
        out.append(9)
    if team > 1:
        out += [64 * S, 64 * S + 1, 192 * S + 1]
    assert max(out) < leng
    return out


def e_tie_sets(S, team, leng):
    """Two slots of a lane; a lane's last slot and the next lane's slot 0; two lanes of a wave; wave 0 and wave 3;
    the two ends; a three-way tie whose smallest node sits in a lower wave than the other two (given in falling order)."""
    sets = [(S + 2, S + 5), (3 * S, 3 * S + 1), (2 * S + 3, 40 * S + 2), (1, leng)]
    if team > 1:
        sets += [(5 * S + 4, 192 * S + 7), (200 * S + 5, 193 * S + 2, 130 * S + 3)]
    return sets


def assert_gpu_takes_expected(case, what, plan=None):
    """trace_batch gives the domains written out from the construction and the bits of their re-score; then, as a
    separate statement, what the CPU trace gives."""
    vit = profile_from_tables(*case.tables)
    try:
        if plan is not None:
            assert vit.trace_describe()["plan"] == plan, what
        batch = _csr([case.codes])
        t = vit.trace_batch(codes=batch[0], offsets=batch[1])
        got = traces_lists(t)[0]
        assert got == case.expected, (what, got, case.expected, case.alternatives)
        assert bits(t.scores[0]) == bits(rescore(*case.tables, case.codes, case.expected)), what
        assert_same(t, [cpu_trace(*case.tables, case.codes)], what)
    finally:
        vit.close()


@pytest.mark.parametrize("plan", range(len(PLANS)))
def test_every_tie_break_rule_at_the_plan_edges(plan):
    """A model of the plan's capacity; every builder case with its tied cell at each anchor of plan_anchors, at the
    first and at the last node its rule allows; E ties inside a lane, across lanes and across waves; and a D tie
    whose losing chain is longer than a lane and crosses a wave boundary (or, in the one-wave plan, two lanes), so
    that the tied value is one that lazy-F propagated over more than one round."""
    name, leng = PLANS[plan]
    S, team = {"vit_trace_s8_w1": (8, 1), "vit_trace_s8_w4": (8, 4), "vit_trace_s16_w4": (16, 4)}[name]
    assert leng == 64 * S * team
    n = 0
    for rule, k, case in anchored_cases(leng, plan_anchors(S, team, leng)):
        prove(case, dp_score=lib_cpu)
        assert_gpu_takes_expected(case, (name, rule, k), plan=name)
        n += 1
    assert n >= len(RULES) * 3
    for ks in e_tie_sets(S, team, leng):
        case = e_takes_the_smallest_k(leng, ks)
        prove(case, dp_score=lib_cpu)
        assert_gpu_takes_expected(case, (name, "E", ks), plan=name)
    edge = 64 * S if team > 1 else 8 * S         # the chain ends three states past a wave (or lane) boundary
    for k, chain in ((edge + 3, 2 * S + 5), (edge + S + 1, 2 * S + 1)):
        case = d_takes_m_before_d(leng, k, chain=chain)
        assert len(case.alternatives[0][0][4]) - 2 > S and case.alternatives[0][0][2] < edge - S
        prove(case, dp_score=lib_cpu)
        assert_gpu_takes_expected(case, (name, "D chain", k, chain), plan=name)


# ---- quantised models: ties by the hundred, the GPU against the CPU trace and against py_trace ----------------------

FUZZ = {24: ("vit_trace_s8_w1", 8, 3), 600: ("vit_trace_s8_w4", 8, 5), 2100: ("vit_trace_s16_w4", 16, 7)}


def fuzz_model_and_batch(leng):
    """A quantised model of LENG `leng` whose match scores take four values, and ~40 sequences of L 1..8 shuffled
    with the edge lengths."""
    seed = FUZZ[leng][2]
    rng = np.random.Generator(np.random.PCG64(seed))
    tables = quantised_model(rng, leng, leng == 600, leng != 24, step=0.5, emissions=(-1.5, -0.5, 0.5, 1.0), depth=1.5)
    seqs = [rng.integers(0, 20, int(rng.integers(1, 9)), dtype=np.uint8) for _ in range(40)]
    ec, eo = edge_batch(seed + 1)
    seqs += [ec[int(eo[i]):int(eo[i + 1])] for i in range(len(eo) - 1)]
    order = rng.permutation(len(seqs))
    return tables, [seqs[int(i)] for i in order]


def e_tie_spread(traces, S):
    """(sequences with an on-path E tie over different lanes, ... over different waves), by py_trace's tied nodes."""
    lanes = sum(any(len(set((nodes - 1) // S)) > 1 for nodes in t.e_tied) for t in traces)
    waves = sum(any(len(set((nodes - 1) // (64 * S))) > 1 for nodes in t.e_tied) for t in traces)
    return lanes, waves


@pytest.mark.parametrize("leng", sorted(FUZZ))
def test_quantised_models(leng):
    """LENG 24 (one wave's first lanes), 600 (the boundary of waves 0 | 1 at 512 | 513 inside the model) and 2,100
    (1,024 | 1,025).  trace_batch == the CPU trace == py_trace; and the batch is not vacuous: by py_trace alone, at
    least 10 sequences tie in E over different lanes, in the team plans at least 5 over different waves."""
    plan, S, _ = FUZZ[leng]
    tables, seqs = fuzz_model_and_batch(leng)
    ref = [py_trace(*tables, s) for s in seqs]
    lanes, waves = e_tie_spread(ref, S)
    tied = sum(t.tied for t in ref)
    counts = f"LENG {leng}: {tied} of {len(seqs)} sequences tied on their path, {lanes} in E over lanes, {waves} over waves"
    print(counts)
    assert lanes >= 10 and (leng == 24 or waves >= 5), counts
    vit = profile_from_tables(*tables)
    try:
        assert vit.trace_describe()["plan"] == plan
        t = check(vit, *_csr(seqs), what=leng)
        got = traces_lists(t)
        for q, r in enumerate(ref):
            assert bits(t.scores[q]) == bits(r.score) and got[q] == r.domains, (counts, q, got[q], r.domains)
    finally:
        vit.close()
