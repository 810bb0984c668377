"""The CPU Viterbi trace (msv_vit_cpu_trace) and the trace's host-only arithmetic (plans, back-pointer layout, chunk
cuts), with no GPU.  Every traced path is checked by trace_check's independent checker: it must be a legal path
of the model, and its float32 left-to-right re-score must have the bits of msv_vit_cpu_score -- on tiny models
also the bits of the best path found by explicit enumeration (test_viterbi_paths.best_path).  Every tie-break rule
of msv.h is pinned by trace_ties' exact-tie cases, and a third trace (trace_check.py_trace) by quantised models."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import hmm_fasta_viterbi_amd as msv
from hmm_fasta_viterbi_amd import _cpu_trace, _native
from hmm_fasta_viterbi_amd.synthetic import gapped_homolog_batch
from oracle_lib import GOLD, PROFILES, ROOT, bits, profile_path
from state_batches import window_core, window_homolog_batch
from test_viterbi_paths import best_path, lib_cpu, random_model
from trace_check import (F, MM, MI, MD, IM, DM, DD, check_legal, cpu_trace, cpu_traces, py_trace, quantised_model,
                         rescore, two_core_batch)
from trace_ties import (ANCHORED_RULES, RULES, anchored_cases, d_takes_m_before_d, e_takes_the_smallest_k, flat_model,
                        prove, smallest_cases, solve)

NINF = F(-np.inf)


def tiny_cases():
    """(msc, isc, tsc, consts, [codes]) of the tiny models: LENG 1..5, inserts off and on, one model in six with
    distinct exits, sequences of L 0..5."""
    for leng in (1, 2, 3, 4, 5):
        for inserts in (False, True):
            rng = np.random.Generator(np.random.PCG64(1000 * leng + inserts))
            for trial in range(6):
                msc, isc, tsc, consts = random_model(rng, leng, inserts)
                if trial == 5:
                    consts = (consts[0], F(consts[1] - F(0.75)), consts[2])
                yield msc, isc, tsc, consts, [rng.integers(0, 20, L, dtype=np.uint8) for L in (0, 1, 2, 3, 4, 4, 5)]


def test_tiny_models_trace_rescore_and_enumeration():
    n = 0
    for msc, isc, tsc, consts, seqs in tiny_cases():
        for codes in seqs:
            sc, doms = cpu_trace(msc, isc, tsc, consts, codes)
            assert bits(sc) == bits(lib_cpu(msc, isc, tsc, consts, codes))
            check_legal(doms, msc.shape[1] - 1, len(codes))
            assert bits(rescore(msc, isc, tsc, consts, codes, doms)) == bits(sc), (doms, sc)
            assert bits(best_path(msc, isc, tsc, consts, codes)) == bits(sc)
            assert (len(doms) == 0) == (len(codes) == 0)
            n += 1
    assert n == 5 * 2 * 6 * 7


# ---- tie-breaks: hand-built models with an exact float tie, the expected trace written out by hand ----------

def test_tie_e_takes_the_smaller_node():
    # two nodes with identical columns, one residue: M(1,1) == M(1,2) == E(1)
    msc, tsc, consts = flat_model(2)
    sc, doms = cpu_trace(msc, None, tsc, consts, np.array([4], np.uint8))
    assert doms == [(1, 1, 1, 1, b"M")]
    assert bits(rescore(msc, None, tsc, consts, [4], doms)) == bits(sc)


def test_tie_m_takes_m_before_b():
    # residues a b on two nodes: M(2,2) = max(M(1,1) + tMM, B(1) + tBM) + e with the two equal
    msc, tsc, consts = flat_model(2)
    msc[0, 1], msc[1, 2] = F(1.0), F(5.0)
    loop, move = (F(x) for x in msv.sequence_transitions(2))
    tBM = consts[0]
    m11 = F(F(move + tBM) + msc[0, 1])
    bt1 = F(F(F(loop) + move) + tBM)            # B(1) = N(1) + move: J is out of reach
    tsc[1, MM] = solve(lambda t: F(m11 + t), bt1, F(bt1 - m11))
    assert tsc[1, MM] <= 0 and F(m11 + tsc[1, MM]) == bt1
    codes = np.array([0, 1], np.uint8)
    sc, doms = cpu_trace(msc, None, tsc, consts, codes)
    assert doms == [(1, 2, 1, 2, b"MM")]        # not (2, 2, 2, 2, b"M"), which scores the same
    assert bits(rescore(msc, None, tsc, consts, codes, doms)) == bits(sc)
    assert bits(rescore(msc, None, tsc, consts, codes, [(2, 2, 2, 2, b"M")])) == bits(sc)


def test_tie_m_takes_m_before_i():
    # residues a b c: M(3,2) = max(M(2,1) + tMM, I(2,1) + tIM, ...) + e with the first two equal
    msc, tsc, consts = flat_model(3)
    msc[0, 1], msc[1, 1], msc[2, 2] = F(3.0), F(1.0), F(6.0)
    tsc[1, MM] = F(-0.25)                       # (so that M(2,1) + tMM beats the entry from B(2))
    loop, move = (F(x) for x in msv.sequence_transitions(3))
    tBM = consts[0]
    m11 = F(F(move + tBM) + msc[0, 1])
    i21 = F(m11 + tsc[1, MI])
    m21 = F(F(F(F(loop) + move) + tBM) + msc[1, 1])
    cm = F(m21 + tsc[1, MM])
    tsc[1, IM] = solve(lambda t: F(i21 + t), cm, F(cm - i21))
    assert tsc[1, IM] <= 0 and F(i21 + tsc[1, IM]) == cm
    codes = np.array([0, 1, 2], np.uint8)
    sc, doms = cpu_trace(msc, None, tsc, consts, codes)
    assert doms == [(2, 3, 1, 2, b"MM")]        # not (1, 3, 1, 2, b"MIM")
    assert bits(rescore(msc, None, tsc, consts, codes, doms)) == bits(sc)
    assert bits(rescore(msc, None, tsc, consts, codes, [(1, 3, 1, 2, b"MIM")])) == bits(sc)


def test_tie_c_takes_the_loop_before_e():
    # one node, residues a b: C(2) = max(C(1) + loop, E(2) + tEC) with the two equal
    msc, tsc, consts = flat_model(1)
    tBM, tEC = consts[0], consts[1]
    msc[0, 1] = F(-2.0)                         # (the tied score is then coarser than the solved match score)
    loop, move = (F(x) for x in msv.sequence_transitions(2))
    cl = F(F(F(F(move + tBM) + msc[0, 1]) + tEC) + loop)
    bt1 = F(F(F(loop) + move) + tBM)
    msc[1, 1] = solve(lambda e: F(F(bt1 + e) + tEC), cl, F(F(cl - tEC) - bt1))
    codes = np.array([0, 1], np.uint8)
    sc, doms = cpu_trace(msc, None, tsc, consts, codes)
    assert doms == [(1, 1, 1, 1, b"M")]         # not the domain at residue 2
    assert bits(rescore(msc, None, tsc, consts, codes, doms)) == bits(sc)
    assert bits(rescore(msc, None, tsc, consts, codes, [(2, 2, 1, 1, b"M")])) == bits(sc)


# ---- all twelve rules through trace_ties' builder, each case proven without either trace ----------------------------

def e_cases(leng):
    """E ties in a model of LENG >= 4: neighbours, the two ends, a three-way tie given in falling order."""
    mid = leng // 2
    return [e_takes_the_smallest_k(leng, ks) for ks in ((mid, mid + 1), (1, leng), (leng, mid, 2))]


def proven(case):
    return prove(case, best_path, lib_cpu)


def assert_cpu_takes_expected(case, what):
    sc = proven(case)
    got_sc, doms = cpu_trace(*case.tables, case.codes)
    assert bits(got_sc) == bits(sc), (what, got_sc, sc)
    assert doms == case.expected, (what, doms, case.expected, case.alternatives)


def test_every_rule_at_its_smallest_model():
    cases = smallest_cases()
    rules = {c.rule for c in cases}
    assert len(rules) == ANCHORED_RULES + 1 == 12, rules
    assert {name.split(",")[0] for name in RULES} | {"E: smallest k"} == rules
    assert sum(c.isc is not None for c in cases) == 2 and max(c.msc.shape[1] - 1 for c in cases) == 4
    for case in cases:
        assert case.msc.shape[1] - 1 <= 5  # (proven against the explicit enumeration)
        assert_cpu_takes_expected(case, case.rule)
    # the C and the J rule on models whose exits differ; B's second domain needs J
    by_rule = {c.rule: c for c in cases}
    for rule in ("C: loop before E", "J: loop before E", "B: N before J"):
        assert by_rule[rule].consts[1] != by_rule[rule].consts[2]
    assert len(by_rule["B: N before J"].alternatives[0]) == 2 and len(by_rule["J: loop before E"].expected) == 2


def test_every_rule_at_the_anchors_of_a_larger_model():
    """LENG 40: the first node a rule allows, the middle, the last (LENG - 1 for the I and the D cell: no I at
    node LENG, no D that ends at the exit).  The solved parameter is the smallest model's: it does not depend on
    the anchor."""
    n = 0
    for name, k, case in anchored_cases(40, (20,)):
        assert_cpu_takes_expected(case, (name, k))
        if case.isc is None:  # (an insert score of the anchor's node enters the solved parameter)
            small = RULES[name].build(max(RULES[name].first + RULES[name].tail, 1), RULES[name].first)
            for a, b in ((case.tsc, small.tsc), (case.msc[:, 1:], small.msc[:, 1:]), (case.consts, small.consts)):
                assert set(bits(a).ravel().tolist()) == set(bits(b).ravel().tolist()), (name, k)
        n += 1
    assert n == 3 * len(RULES)
    for rule in ("I: M before I", "D: M before D"):
        assert max(k for name, k, _ in anchored_cases(40, ()) if name == rule) == 39
    for case in e_cases(40):
        assert_cpu_takes_expected(case, case.rule)
    assert_cpu_takes_expected(d_takes_m_before_d(40, 30, chain=21), "D chain")


def builder_cases():
    return smallest_cases() + [c for _, _, c in anchored_cases(40, (20,))] + e_cases(40)


def assert_py_equals_cpu(tables, codes, what):
    """py_trace against cpu_trace: score bits, domains and ops.  Returns py_trace's result."""
    sc, doms = cpu_trace(*tables, codes)
    t = py_trace(*tables, codes)
    assert bits(t.score) == bits(sc), (what, t.score, sc)
    assert t.domains == doms, (what, t.domains, doms)
    return t


def test_py_trace_equals_the_cpu_trace_on_tiny_models_and_builder_cases():
    n = 0
    for msc, isc, tsc, consts, seqs in tiny_cases():
        for codes in seqs:
            assert_py_equals_cpu((msc, isc, tsc, consts), codes, n)
            n += 1
    assert n == 5 * 2 * 6 * 7
    for case in builder_cases():
        t = assert_py_equals_cpu(case.tables, case.codes, case.rule)
        assert t.domains == case.expected
        assert t.ties[case.rule[0]] >= 1, (case.rule, t.ties)  # py_trace sees the planted tie, under its rule


FUZZ_SEQUENCES = 1500


def test_quantised_models_cpu_trace_equals_py_trace():
    """Seeded models whose every score is a multiple of 0.25 or 0.5 from [-1.5, 0.75] or [-1, 0.5]: LENG 3..12,
    L 2..10, half with distinct exits, insert scores on for a third, every other model periodic in its nodes (low
    complexity).  The share of sequences with an on-path tie, counted by py_trace alone,
    must be at least one in five (measured: see the assertion's message) -- else the comparison pins nothing."""
    rng = np.random.Generator(np.random.PCG64(2024))
    n = tied = 0
    by_rule = dict.fromkeys("MIDECJB", 0)
    model = 0
    while n < FUZZ_SEQUENCES:
        leng = int(rng.integers(3, 13))
        tables = quantised_model(rng, leng, model % 3 == 0, model // 2 % 2 == 1, step=0.25 if model // 4 % 2 else 0.5,
                                 depth=1.0 if model // 8 % 2 else 1.5,
                                 period=int(rng.integers(1, leng)) if model % 2 == 0 else None)
        model += 1
        for _ in range(10):
            codes = rng.integers(0, 20, int(rng.integers(2, 11)), dtype=np.uint8)
            t = assert_py_equals_cpu(tables, codes, (model, n))
            check_legal(t.domains, leng, len(codes))
            assert bits(rescore(*tables, codes, t.domains)) == bits(t.score)
            tied += t.tied
            for rule, c in t.ties.items():
                by_rule[rule] += c > 0
            n += 1
    print(f"quantised fuzz: {tied} of {n} sequences with an on-path tie; per rule {by_rule}")
    assert 5 * tied >= n, (tied, n, by_rule)
    assert all(by_rule[r] > 0 for r in "MIDEC"), by_rule


# ---- bundled profiles ---------------------------------------------------------------------------------------

_engines = {}


def host_tables(prof, insert_mode=0):
    """Tables of a bundled profile without a device (msv_hmm_viterbi_scores on the parse)."""
    key = (prof, insert_mode)
    if key not in _engines:
        hmm = msv.Profile_HMM(profile_path(prof))
        M = hmm.model_length
        msc, isc, tsc = np.zeros((20, M), F), np.zeros((20, M), F), np.zeros((M, 7), F)
        b, c, j = C.c_float(), C.c_float(), C.c_float()
        assert _native.lib().msv_hmm_viterbi_scores(hmm._h, insert_mode, msc.ctypes.data, isc.ctypes.data,
                                                    tsc.ctypes.data, C.byref(b), C.byref(c), C.byref(j)) == 0
        _engines[key] = (hmm, (msc, isc if insert_mode else None, tsc, (b.value, c.value, j.value)))
    return _engines[key]


@pytest.mark.parametrize("prof", PROFILES)
def test_bundled_profiles_traces_are_legal_and_rescore(prof):
    hmm, tables = host_tables(prof)
    k = prof.split(".")[0]
    z = np.load(os.path.join(GOLD, "seeded_all_profiles.npz"))
    batches = [(z[f"codes_{k}"], z[f"offsets_{k}"]),
               gapped_homolog_batch(hmm.match_emissions, 31, 6, 40, 160)]
    used = set()
    for codes, offsets in batches:
        for s, (sc, doms) in enumerate(cpu_traces(tables, codes, offsets)):
            seq = codes[int(offsets[s]):int(offsets[s + 1])]
            assert bits(sc) == bits(lib_cpu(*tables, seq))
            check_legal(doms, hmm.model_length - 1, len(seq))
            assert bits(rescore(*tables, seq, doms)) == bits(sc), (prof, s)
            for d in doms:
                used |= set(d[4])
    assert 77 in used


def stress_tables(tables):
    """test_team_variant_stress's transitions (d->d 0.995, m->d 0.3, d->m 0.9): long D chains are cheap."""
    msc, isc, tsc, consts = tables
    t = tsc.copy()
    t[:, DD], t[:, MD], t[:, DM] = F(np.log(F(0.995))), F(np.log(F(0.3))), F(np.log(F(0.9)))
    return msc, isc, t, consts


def test_ops_cover_m_i_and_d():
    """The checks above are not vacuous for I and D: the golden seeded sequences put I on best paths of 100.hmm, and
    gapped homologs under the lazy-F stress transitions D on those of 1400.hmm."""
    used = set()
    for prof, tables in (("100.hmm", host_tables("100.hmm")[1]),
                         ("1400.hmm", stress_tables(host_tables("1400.hmm")[1]))):
        hmm = host_tables(prof)[0]
        if prof == "100.hmm":
            z = np.load(os.path.join(GOLD, "seeded_all_profiles.npz"))
            codes, offsets = z["codes_100"], z["offsets_100"]
        else:
            codes, offsets = gapped_homolog_batch(hmm.match_emissions, 31, 6, 40, 160)
        for s, (sc, doms) in enumerate(cpu_traces(tables, codes, offsets)):
            seq = codes[int(offsets[s]):int(offsets[s + 1])]
            check_legal(doms, hmm.model_length - 1, len(seq))
            assert bits(rescore(*tables, seq, doms)) == bits(sc) == bits(lib_cpu(*tables, seq))
            for d in doms:
                used |= set(d[4])
    assert used == {77, 73, 68}, used


@pytest.mark.parametrize("prof,seed", [("100.hmm", 5), ("1400.hmm", 5), ("2405.hmm", 5)])
def test_planted_windows_are_found(prof, seed):
    """A core emitted by a window of states: some domain of the trace runs through the window, for EVERY
    sequence of these seeds."""
    hmm, tables = host_tables(prof)
    leng = hmm.model_length - 1
    starts = [0, 60, leng // 2, leng - 30, leng - 24]
    codes, offsets = window_homolog_batch(hmm.match_emissions, seed, starts, 24)
    for s, (sc, doms) in enumerate(cpu_traces(tables, codes, offsets)):
        lo, hi = window_core(starts[s], 24, leng)
        assert any(d[2] <= hi and d[3] >= lo for d in doms), (prof, s, (lo, hi), doms)


def test_two_cores_give_two_domains():
    """Two planted cores with a spacer: with seed 3 on 1400.hmm, 2 of the 8 sequences have two domains (found on
    the CPU); at least one must, and every path re-scores to the score."""
    hmm, tables = host_tables("1400.hmm")
    codes, offsets = two_core_batch(hmm.match_emissions, 3, 8)
    counts = []
    for s, (sc, doms) in enumerate(cpu_traces(tables, codes, offsets)):
        seq = codes[int(offsets[s]):int(offsets[s + 1])]
        check_legal(doms, hmm.model_length - 1, len(seq))
        assert bits(rescore(*tables, seq, doms)) == bits(sc)
        counts.append(len(doms))
    assert max(counts) >= 2, counts
    assert sum(c >= 2 for c in counts) == TWO_DOMAIN_SEQUENCES, counts


TWO_DOMAIN_SEQUENCES = 2


# ---- the remaining host checks -------------------------------------------------------------------------------

def test_sizing_protocol_and_bad_residue():
    hmm, tables = host_tables("100.hmm")
    msc, isc, tsc, consts = tables
    codes, offsets = gapped_homolog_batch(hmm.match_emissions, 2, 1, 120, 120)
    L = _native.lib()
    sc, nd, no = C.c_float(), C.c_uint32(), C.c_uint64()
    args = (msc.ctypes.data, None, tsc.ctypes.data, msc.shape[1], *consts, codes.ctypes.data, codes.size)
    assert L.msv_vit_cpu_trace(*args, C.byref(sc), C.byref(nd), C.byref(no), None, None) == 0
    assert nd.value >= 1 and no.value >= nd.value
    doms = np.zeros(nd.value, _native.DOMAIN_DTYPE)
    ops = np.zeros(no.value, np.uint8)
    assert L.msv_vit_cpu_trace(*args, C.byref(sc), C.byref(nd), C.byref(no), doms.ctypes.data, ops.ctypes.data) == 0
    assert int(doms["ops_len"].sum()) == no.value and int(doms["ops_begin"][0]) == 0
    assert bits(F(sc.value)) == bits(lib_cpu(msc, None, tsc, consts, codes))
    # buffers too small for the second call, and one buffer without the other
    small = C.c_uint64(no.value - 1)
    assert L.msv_vit_cpu_trace(*args, C.byref(sc), C.byref(nd), C.byref(small), doms.ctypes.data,
                               ops.ctypes.data) == 1
    assert L.msv_vit_cpu_trace(*args, C.byref(sc), C.byref(nd), C.byref(no), doms.ctypes.data, None) == 1
    # a bad residue: the score call's status
    bad = codes.copy()
    bad[7] = 23
    st, _, _, _ = _cpu_trace(msc, None, tsc, consts, bad)
    assert st == _native.MSV_ERR_BAD_RESIDUE
    out = C.c_float()
    assert L.msv_vit_cpu_score(msc.ctypes.data, None, tsc.ctypes.data, msc.shape[1], *consts, bad.ctypes.data,
                               bad.size, C.byref(out)) == _native.MSV_ERR_BAD_RESIDUE


def chunk_cuts(sizes, workspace):
    L = _native.lib()
    b = np.ascontiguousarray(sizes, np.uint64)
    cuts = np.zeros(len(b) + 1, np.uint64)
    n = C.c_uint64()
    st = L.msv_vit_trace_chunk_cuts(b.ctypes.data if b.size else None, b.size, workspace, cuts.ctypes.data,
                                    C.byref(n))
    return st, [int(x) for x in cuts[:n.value + 1]]


def test_chunk_cuts():
    rng = np.random.Generator(np.random.PCG64(11))
    for trial in range(200):
        n = int(rng.integers(0, 40))
        sizes = rng.integers(0, 1000, n).astype(np.uint64)
        workspace = int(rng.integers(1, 3000))
        st, cuts = chunk_cuts(sizes, workspace)
        if n and sizes.max() > workspace:
            assert st == 9  # MSV_ERR_OUT_OF_MEMORY: an oversize sequence is refused
            continue
        assert st == 0
        # every selected sequence lands in exactly one chunk, in order; no chunk goes over the workspace
        assert cuts[0] == 0 and cuts[-1] == n and all(a < b for a, b in zip(cuts, cuts[1:])), cuts
        assert (len(cuts) - 1 == 0) == (n == 0)
        for a, b in zip(cuts, cuts[1:]):
            assert int(sizes[a:b].sum()) <= workspace
            # greedy: the next sequence did not fit
            assert b == n or int(sizes[a:b + 1].sum()) > workspace
    assert chunk_cuts([5, 5, 5], 5) == (0, [0, 1, 2, 3])
    assert chunk_cuts([5, 5, 5], 4)[0] == 9
    assert chunk_cuts([2 ** 63, 2 ** 63], 2 ** 64 - 1) == (0, [0, 1, 2])  # the sum does not wrap


def test_pointer_word_layout():
    L = _native.lib()
    plans = msv.Viterbi_HMM.trace_plans()
    assert [c for _, c in plans] == sorted(c for _, c in plans) and plans[-1][1] >= 4096
    for i, (name, cap) in enumerate(plans):
        out = [C.c_uint32() for _ in range(5)]
        refs = [C.byref(x) for x in out]
        assert L.msv_vit_trace_plan_cell(i, 1, *refs) == 0
        words, lanes = out[3].value, out[4].value
        S = cap // lanes
        assert lanes % 64 == 0 and S * lanes == cap and words == (S + 7) // 8
        for states in (cap, cap - 1, 1):   # models of capacity, capacity - 1 and 1 real states
            seen = set()
            for k in range(1, states + 1):
                assert L.msv_vit_trace_plan_cell(i, k, *refs) == 0
                w, l, sh = (x.value for x in out[:3])
                assert w < words and l < lanes and sh % 4 == 0 and sh <= 28
                assert l == (k - 1) // S and w * 8 + sh // 4 == (k - 1) % S  # S consecutive states per lane
                seen.add((w, l, sh))
            assert len(seen) == states     # no two nodes share their 4 bits
        assert L.msv_vit_trace_plan_cell(i, 0, *refs) == 1 and L.msv_vit_trace_plan_cell(i, cap + 1, *refs) == 1
        for rows in (0, 1, 400):
            assert L.msv_vit_trace_sequence_bytes(i, rows) == rows * (words * lanes + 1) * 4
    assert L.msv_vit_trace_plan_cell(len(plans), 1, *refs) == 1


def test_asan_trace():
    """tests/cpp/sanitize_trace.cpp under AddressSanitizer + UBSan: the CPU trace, the chunk cuts and the layout,
    built from the host-only sources (no code loaded into Python is run under a sanitizer)."""
    p = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "hmm_fasta_viterbi_amd", "csrc"), "asan_trace"],
                       capture_output=True, text=True, timeout=900)
    out = p.stdout + p.stderr
    assert p.returncode == 0, out[-4000:]
    assert "sanitize_trace passed" in out
    assert "ERROR: AddressSanitizer" not in out and "runtime error:" not in out
