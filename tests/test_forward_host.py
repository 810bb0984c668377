"""The Forward stage on the host: msv_fwd_cpu_score -- float64, the reference of every GPU test --
against an independent numpy float64 recurrence in log space (forward_lib.np_forward), its relation to the Viterbi
score, its edge cases, the P-value formula and the D-scan constants the device layer uploads.  It also shows, with
the numpy recurrence, that every term of the model carries weight far above the GPU tolerance on the model the GPU
tests use for it -- the tolerance is loose, so a kernel that dropped a term must not be able to hide under it."""
import ctypes as C
import os

import numpy as np
import pytest

import hmm_fasta_viterbi_amd as msv
from hmm_fasta_viterbi_amd import _native
from hmm_fasta_viterbi_amd.synthetic import (concat_batches, gapped_homolog_batch, homolog_batch, random_batch)
from forward_lib import (DD, cpu_score, cpu_scores, distinct_exits, np_forward, stress_transitions, tables, tolerance)
from oracle_lib import PROFILES, ROOT, profile_path
from sparse_lane_batches import SLOTS, sparse_lengths

_hmm = {}


def hmm(prof):
    if prof not in _hmm:
        _hmm[prof] = msv.Profile_HMM(profile_path(prof))
    return _hmm[prof]


def split(codes, offsets):
    return [codes[int(offsets[i]):int(offsets[i + 1])] for i in range(len(offsets) - 1)]


def small_batch(prof, seed, n_each, lmin, lmax):
    me = hmm(prof).match_emissions
    return concat_batches(random_batch(seed, n_each, lmin, lmax), homolog_batch(me, seed + 1, n_each, lmin, lmax),
                          gapped_homolog_batch(me, seed + 2, n_each, lmin, lmax))


def stress_model(prof):
    msc, isc, tsc, consts = tables(hmm(prof), 0)
    return msc, None, stress_transitions(tsc), distinct_exits(consts)


@pytest.mark.parametrize("prof,mode", [("100.hmm", 0), ("100.hmm", 1), ("300.hmm", 0), ("300.hmm", 1)])
def test_cpu_forward_equals_the_numpy_recurrence(prof, mode):
    msc, isc, tsc, consts = tables(hmm(prof), mode)
    codes, offsets = concat_batches(small_batch(prof, 11, 2, 1, 90), random_batch(3, 2, 1, 3))
    got = cpu_scores(msc, isc, tsc, consts, codes, offsets)
    for q, s in enumerate(split(codes, offsets)):
        want = np_forward(msc, isc, tsc, consts, s)
        assert abs(got[q] - want) <= 1e-9 * max(1.0, abs(want)), (prof, mode, q, got[q], want)


@pytest.mark.parametrize("prof,lmax", [("300.hmm", 90), ("1400.hmm", 40)])
def test_cpu_forward_equals_the_numpy_recurrence_on_the_stress_models(prof, lmax):
    msc, isc, tsc, consts = stress_model(prof)
    codes, offsets = small_batch(prof, 13, 1, lmax // 2, lmax)
    got = cpu_scores(msc, isc, tsc, consts, codes, offsets)
    for q, s in enumerate(split(codes, offsets)):
        want = np_forward(msc, isc, tsc, consts, s)
        assert abs(got[q] - want) <= 1e-9 * max(1.0, abs(want)), (prof, q, got[q], want)


@pytest.mark.parametrize("prof", PROFILES)
def test_forward_is_at_least_viterbi(prof):
    """The sum over every path is at least its largest term.  The Viterbi score is float32 arithmetic along one path
    of at most 3 (L + LENG) adds, each rounding at most 2^-24 of a partial sum bounded by |score| + 20 nats."""
    fa = msv.FASTA_protein_sequences(os.path.join(ROOT, "data", "FASTA_files", "fasta_like_example.fsa"))
    msc, isc, tsc, consts = tables(hmm(prof), 0)
    fwd = cpu_scores(msc, None, tsc, consts, fa.codes, fa.offsets)
    for q, s in enumerate(split(fa.codes, fa.offsets)):
        v = C.c_float()
        assert _native.lib().msv_vit_cpu_score(msc.ctypes.data, None, tsc.ctypes.data, msc.shape[1], *consts,
                                               s.ctypes.data, len(s), C.byref(v)) == 0
        slack = 3 * (len(s) + msc.shape[1]) * 2.0 ** -24 * (abs(v.value) + 20.0)
        assert fwd[q] >= v.value - slack, (prof, q, fwd[q], v.value)


def test_edge_cases():
    msc, isc, tsc, consts = tables(hmm("100.hmm"), 0)
    st, sc = cpu_score(msc, None, tsc, consts, np.zeros(0, np.uint8))
    assert st == 0 and sc == -np.inf
    st, _ = cpu_score(msc, None, tsc, consts, np.array([3, 20, 4], np.uint8))
    assert st == _native.MSV_ERR_BAD_RESIDUE
    st, _ = cpu_score(msc, None, tsc, consts, np.array([255], np.uint8))
    assert st == _native.MSV_ERR_BAD_RESIDUE
    out = C.c_double()
    assert _native.lib().msv_fwd_cpu_score(None, None, tsc.ctypes.data, 101, 0.0, 0.0, 0.0, None, 0, C.byref(out)) == 1
    # a batch keeps the order and scores the empty sequence too
    codes, offsets = random_batch(5, 6, 0, 40)
    got = cpu_scores(msc, None, tsc, consts, codes, offsets)
    for q, s in enumerate(split(codes, offsets)):
        assert got[q] == cpu_score(msc, None, tsc, consts, s)[1]


def test_long_homologs_pass_the_float64_rescaling():
    """A score beyond float64's own odds range (709 nats) comes back finite and equal to the log-space recurrence."""
    prof = "100.hmm"
    msc, isc, tsc, consts = tables(hmm(prof), 0)
    core, o = homolog_batch(hmm(prof).match_emissions, 3, 1, 100, 100, mutate=0.0)
    s = np.tile(core, 70)  # (about 12 nats per copy)
    st, got = cpu_score(msc, None, tsc, consts, s)
    assert st == 0 and np.isfinite(got) and got > 709.0
    want = np_forward(msc, None, tsc, consts, s)
    assert abs(got - want) <= 1e-9 * abs(want)


# ---- every term carries weight far above the GPU tolerance, on the model the GPU tests use for it ----------------

def moved(full, without, L, leng):
    """Per sequence: |score - score without the term| in units of the GPU tolerance."""
    return np.abs(np.asarray(full) - np.asarray(without)) / tolerance(L, leng, np.asarray(full))


def term_weights(model, seqs, **switch):
    msc, isc, tsc, consts = model
    full = [np_forward(msc, isc, tsc, consts, s) for s in seqs]
    cut = [np_forward(msc, isc, tsc, consts, s, **switch) for s in seqs]
    return moved(full, cut, [len(s) for s in seqs], msc.shape[1] - 1)


def test_term_d_exits_on_the_stress_model():
    model = stress_model("300.hmm")
    codes, offsets = small_batch("300.hmm", 17, 1, 40, 80)
    w = term_weights(model, split(codes, offsets), d_exits=False)
    print("D -> E exits: moved by", w, "tolerances")
    assert w.min() > 100.0


def test_term_dm_on_the_stress_model():
    model = stress_model("300.hmm")
    codes, offsets = small_batch("300.hmm", 17, 1, 40, 80)
    w = term_weights(model, split(codes, offsets), dm=False)
    print("d->m: moved by", w, "tolerances")
    assert w.min() > 100.0


def test_term_cross_lane_d_chains_on_the_stress_model():
    """D mass that entered its chain more than 64 states upstream -- in the kernel it has crossed at least two lane
    boundaries (S <= 38), so only the cross-lane scan can deliver it."""
    model = stress_model("1400.hmm")
    codes, offsets = small_batch("1400.hmm", 19, 1, 20, 40)
    w = term_weights(model, split(codes, offsets), d_reach=64)
    print("D from > 64 states upstream: moved by", w, "tolerances")
    assert w.min() > 100.0
    # the cut recurrence is the full one when nothing is cut
    msc, isc, tsc, consts = model
    s = split(codes, offsets)[0]
    assert abs(np_forward(msc, isc, tsc, consts, s, d_reach=1400) - np_forward(msc, isc, tsc, consts, s)) < 1e-9


def test_term_i_states_on_gapped_homologs_with_insert_scores():
    prof = "100.hmm"
    model = tables(hmm(prof), 1)
    codes, offsets = gapped_homolog_batch(hmm(prof).match_emissions, 23, 6, 60, 100, p_insert=0.08)
    w = term_weights(model, split(codes, offsets), inserts=False)
    print("I states: moved by", w, "tolerances")
    assert np.sum(w > 100.0) >= 3


def test_term_j_loop_on_repeated_homologs():
    prof = "100.hmm"
    model = tables(hmm(prof), 0)
    core, _ = homolog_batch(hmm(prof).match_emissions, 29, 1, 60, 60, mutate=0.0)
    w = term_weights(model, [np.tile(core, 2), np.tile(core, 3)], j_loop=False)
    print("J loop: moved by", w, "tolerances")
    assert w.min() > 100.0


def test_asan_forward():
    """tests/cpp/sanitize_forward.cpp under AddressSanitizer + UBSan: the CPU Forward, the table builders at exact
    fit and the P-values, built from the host-only sources (no code loaded into Python is run under a sanitizer)."""
    import subprocess
    p = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "hmm_fasta_viterbi_amd", "csrc"), "asan_forward"],
                       capture_output=True, text=True, timeout=900)
    out = p.stdout + p.stderr
    assert p.returncode == 0, out[-4000:]
    assert "sanitize_forward passed" in out
    assert "ERROR: AddressSanitizer" not in out and "runtime error:" not in out


def test_fwd_info_layout_matches_the_header(tmp_path):
    """The ctypes mirror of msv_fwd_info has the C header's field offsets and size (gcc on include/msv.h)."""
    import subprocess
    py = _native.FwdInfo
    src = ['#include <stddef.h>', '#include <stdio.h>', '#include "msv.h"', "int main(void) {",
           '  printf("size %zu\\n", sizeof(msv_fwd_info));']
    src += [f'  printf("{f} %zu\\n", offsetof(msv_fwd_info, {f}));' for f, _ in py._fields_]
    src.append("  return 0; }")
    (tmp_path / "layout.c").write_text("\n".join(src))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", f"-I{os.path.join(ROOT, 'include')}", str(tmp_path / "layout.c"), "-o", str(exe)],
                   check=True, capture_output=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True,
                                                       check=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(py)
    for f, _ in py._fields_:
        assert int(got[f]) == getattr(py, f).offset, f


# ---- P-values and the scan constants ---------------------------------------------------------------------------

def test_pvalues_against_a_float64_restatement():
    rng = np.random.Generator(np.random.PCG64(31))
    n = 200
    lengths = rng.integers(1, 3000, n)
    lengths[:3] = [0, 1, 100000]
    offsets = np.zeros(n + 1, np.uint64)
    np.cumsum(lengths, out=offsets[1:])
    scores = rng.normal(-2.0, 8.0, n).astype(np.float32)
    scores[0] = -np.inf
    scores[5] = np.inf
    scores[6] = -np.inf
    tau, lam = np.float32(-4.1234), np.float32(0.71)
    out = np.zeros(n)
    assert _native.lib().msv_fwd_pvalues(scores.ctypes.data, offsets.ctypes.data, n, tau, lam, out.ctypes.data) == 0
    for i in range(n):
        L = int(lengths[i])
        if L == 0:
            assert out[i] == 1.0
            continue
        p1 = np.float32(L) / np.float32(L + 1)
        nullsc = np.float32(L * np.log(np.float64(p1)) + np.log(1.0 - np.float64(p1)))
        bits = np.float32(np.float32(scores[i] - nullsc) / np.float32(0.69314718055994529))
        want = 1.0 if bits < tau else np.exp(-np.float64(lam) * (np.float64(bits) - np.float64(tau)))
        assert out[i] == pytest.approx(want, rel=1e-12, abs=0.0), (i, out[i], want)
    assert out[5] == 0.0 and out[6] == 1.0
    assert np.all((out >= 0.0) & (out <= 1.0))
    bad = np.array([0, 5, 2], np.uint64)
    assert _native.lib().msv_fwd_pvalues(scores.ctypes.data, bad.ctypes.data, 2, tau, lam, out.ctypes.data) == 1


SCAN_CASES = [(1, 2), (65, 2), (128, 2), (300, 6), (1400, 22), (1407, 22), (2432, 38)]
# the sparse-lane lengths of every S, each once ((65, 2) is above already; 385 is two of S = 12's three)
SCAN_CASES += [c for c in dict.fromkeys((leng, S) for S in SLOTS for leng in sparse_lengths(S)) if c not in SCAN_CASES]


@pytest.mark.parametrize("leng,S", SCAN_CASES)
def test_scan_constants_against_cumprod(leng, S):
    rng = np.random.Generator(np.random.PCG64(leng))
    M = leng + 1
    tsc = np.log(rng.uniform(0.05, 1.0, (M, 7))).astype(np.float32)
    dd, prefix, steps = np.zeros((64, S), np.float32), np.zeros((64, S), np.float32), np.zeros((6, 64), np.float32)
    assert _native.lib().msv_fwd_scan_constants(tsc.ctypes.data, M, S, dd.ctypes.data, prefix.ctypes.data,
                                                steps.ctypes.data) == 0
    # slot q of lane l is state k = l S + q + 1; the d->d into it is node k-1's, for k = 2 .. LENG
    want_dd = np.zeros(64 * S)
    k = np.arange(1, 64 * S + 1)
    real = (k >= 2) & (k <= leng)
    want_dd[real] = np.exp(tsc[k[real] - 1, DD].astype(np.float64))
    assert np.array_equal(dd.ravel(), want_dd.astype(np.float32))
    lanes = dd.astype(np.float64)
    np.testing.assert_allclose(prefix, np.cumprod(lanes, axis=1), rtol=2.0 ** -23, atol=1e-45)
    whole = np.cumprod(lanes, axis=1)[:, -1]
    for j in range(6):
        want = np.array([np.prod(whole[max(0, l - 2 ** j + 1):l + 1]) for l in range(64)])
        np.testing.assert_allclose(steps[j], want, rtol=2.0 ** -23, atol=1e-45)
    # padding: the prefix product of every slot beyond LENG, and every step's multiplier of a lane whose window
    # max(0, l - 2^j + 1) .. l holds a padding lane (lane l itself from LENG // S on), are exactly 0.0
    assert not prefix.ravel()[leng:].any() and not steps[:, leng // S:].any()
    assert _native.lib().msv_fwd_scan_constants(tsc.ctypes.data, M, 3, None, None, None) == 1  # odd S
    if leng > 128:
        assert _native.lib().msv_fwd_scan_constants(tsc.ctypes.data, M, 2, None, None, None) == 1  # S too small
