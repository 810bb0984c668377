"""The domain stage on the host: msv_dom_cpu_decode -- float64, the reference of every GPU test -- against
its own Forward (Backward must give the same score), against an independent numpy log-space restatement with full
matrices (occ counted on the core states), the envelope rule on hand-built arrays, the mirrored D-scan constants the
device layer uploads, the describe struct's layout, and the host half under the sanitizers."""
import ctypes as C
import os

import numpy as np
import pytest

import hmm_fasta_viterbi_amd as msv
from hmm_fasta_viterbi_amd import _native
from hmm_fasta_viterbi_amd.synthetic import concat_batches, gapped_homolog_batch, homolog_batch, random_batch
from decode_lib import cpu_decode, cpu_decode_batch, np_decode
from forward_lib import DD, cpu_scores, tables
from oracle_lib import PROFILES, ROOT, profile_path
from sparse_lane_batches import SLOTS, sparse_lengths

_hmm = {}


def hmm(prof):
    if prof not in _hmm:
        _hmm[prof] = msv.Profile_HMM(profile_path(prof))
    return _hmm[prof]


def split(codes, offsets):
    return [codes[int(offsets[i]):int(offsets[i + 1])] for i in range(len(offsets) - 1)]


@pytest.mark.parametrize("prof", PROFILES)
def test_backward_equals_forward_on_the_bundled_profiles(prof):
    """Homolog, gapped and background sequences: the Backward score is the Forward score (to 1e-9 relative), which is
    msv_fwd_cpu_score's; sum begin = sum end (a domain that begins ends); every posterior lies in [0, 1]."""
    me = hmm(prof).match_emissions
    model = tables(hmm(prof), 0)
    codes, offsets = concat_batches(random_batch(41, 2, 30, 120), homolog_batch(me, 42, 2, 60, 150),
                                    gapped_homolog_batch(me, 43, 2, 60, 150))
    fwd, bck, begin, end, occ = cpu_decode_batch(*model, codes, offsets)
    want = cpu_scores(*model, codes, offsets)
    assert np.all(np.abs(fwd - want) <= 1e-12 * np.abs(want))
    assert np.all(np.abs(bck - fwd) <= 1e-9 * np.maximum(1.0, np.abs(fwd))), (prof, bck - fwd)
    off = offsets.astype(np.int64)
    for s in range(len(off) - 1):
        b, e, o = (x[off[s]:off[s + 1]] for x in (begin, end, occ))
        assert abs(b.sum() - e.sum()) <= 1e-9 * max(1.0, b.sum()), (prof, s)
        assert b.min() >= 0.0 and e.min() >= 0.0 and o.min() >= -1e-12 and o.max() <= 1.0 + 1e-12


def test_backward_equals_forward_through_the_rescaling():
    """A 6,000-residue chain of homologs: both passes rescale many times (the score is beyond float64's own odds
    range) and still agree."""
    prof = "100.hmm"
    model = tables(hmm(prof), 0)
    core, _ = homolog_batch(hmm(prof).match_emissions, 3, 1, 100, 100, mutate=0.0)
    s = np.tile(core, 60)
    assert len(s) == 6000
    st, fwd, bck, begin, end, occ = cpu_decode(*model, s)
    assert st == 0 and fwd > 600.0 and abs(bck - fwd) <= 1e-9 * fwd
    assert abs(begin.sum() - end.sum()) <= 1e-9 * begin.sum() and begin.sum() > 30.0
    assert occ.min() >= -1e-12 and occ.max() <= 1.0 + 1e-12


@pytest.mark.parametrize("prof,mode", [("100.hmm", 0), ("100.hmm", 1), ("200.hmm", 0)])
def test_cpu_decode_equals_the_numpy_restatement(prof, mode):
    """begin / end / occ against the log-space restatement, and occ -- computed on the specials -- against the same
    probability counted on the core states: sum_k (fM bM + fI bI) / Z."""
    model = tables(hmm(prof), mode)
    me = hmm(prof).match_emissions
    codes, offsets = concat_batches(random_batch(51, 1, 20, 40), homolog_batch(me, 52, 1, 50, 70),
                                    gapped_homolog_batch(me, 53, 1, 50, 70))
    for s in split(codes, offsets):
        st, fwd, bck, begin, end, occ = cpu_decode(*model, s)
        ref = np_decode(*model, s)
        assert st == 0 and abs(fwd - ref["fwd"]) <= 1e-9 * abs(fwd) and abs(bck - ref["bck"]) <= 1e-9 * abs(bck)
        for name, got in (("begin", begin), ("end", end), ("occ", occ)):
            assert np.all(np.abs(got - ref[name]) <= 1e-9), (prof, mode, name)
        assert np.all(np.abs(occ - ref["occ_core"]) <= 1e-9), np.abs(occ - ref["occ_core"]).max()


def test_edge_cases():
    model = tables(hmm("100.hmm"), 0)
    st, fwd, bck, *_ = cpu_decode(*model, np.zeros(0, np.uint8))
    assert st == 0 and fwd == -np.inf and bck == -np.inf
    assert cpu_decode(*model, np.array([3, 20, 4], np.uint8))[0] == _native.MSV_ERR_BAD_RESIDUE
    st, fwd, bck, begin, end, occ = cpu_decode(*model, np.array([7], np.uint8))
    assert st == 0 and abs(fwd - bck) <= 1e-12 * abs(fwd) and begin.shape == (1,) and abs(begin[0] - end[0]) <= 1e-12
    engine_free = msv.dom_regions(np.zeros(0), np.zeros(0), np.zeros(0))
    assert len(engine_free) == 0


# ---- the envelope rule on hand-built arrays ------------------------------------------------------------------------

def regions(begin, end, occ, **kw):
    return [(int(r["i_from"]), int(r["i_to"])) for r in msv.dom_regions(begin, end, occ, **kw)]


def test_rule_region_open_at_L_is_not_emitted():
    occ = np.array([0.0, 0.9, 0.9, 0.9], np.float32)
    z = np.zeros(4, np.float32)
    assert regions(z, z, occ) == []
    end = np.array([0.0, 0.0, 0.0, 0.85], np.float32)
    assert regions(z, end, occ) == [(1, 4)]  # start: the first residue scanned, never moved (occ - begin >= rt2 from 2)


def test_rule_back_to_back_regions_and_sums():
    occ = np.array([0.0, 0.3, 0.9, 0.9, 0.2, 0.9, 0.9, 0.05, 0.9, 0.9], np.float32)
    begin = np.array([0.0, 0.3, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.8, 0.0], np.float32)
    end = np.array([0.0, 0.0, 0.0, 0.85, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0], np.float32)
    r = msv.dom_regions(begin, end, occ)
    assert [(int(x["i_from"]), int(x["i_to"])) for x in r] == [(2, 4), (5, 8)]
    # serial float32 sums in index order
    f = np.float32
    assert r[0]["expected_domains"] == f(f(f(0.3) + f(0.0)) + f(0.0))
    assert r[0]["mass"] == f(f(f(0.3) + f(0.9)) + f(0.9))
    assert r[1]["mass"] == f(f(f(f(0.2) + f(0.9)) + f(0.9)) + f(0.05))
    assert np.all(r["seq"] == 0)


def test_rule_thresholds_are_inclusive_as_stated():
    z = np.zeros(3, np.float32)
    # occ exactly at rt1 triggers (>=); just below does not
    end = np.array([0.0, 0.0, 0.25], np.float32)
    assert regions(z, end, np.array([0.0, 0.25, 0.25], np.float32)) == [(1, 3)]
    below = np.nextafter(np.float32(0.25), np.float32(0))
    assert regions(z, end, np.array([0.0, below, below], np.float32)) == []
    # occ - end exactly at rt2 does not close (<); just below does
    # (rt2 = 1/8, so that the difference is exact in float32)
    occ = np.array([0.5, 0.5, 0.5], np.float32)
    at = np.array([0.0, 0.375, 0.0], np.float32)
    assert np.float32(0.5) - at[1] == np.float32(0.125)
    assert regions(z, at, occ, rt2=0.125) == []
    at[1] = np.nextafter(at[1], np.float32(1))
    assert regions(z, at, occ, rt2=0.125) == [(1, 2)]
    # the parameters are the caller's
    assert regions(z, end, np.array([0.0, 0.25, 0.25], np.float32), rt1=0.3) == []


def test_rule_start_is_moved_forward_by_the_first_branch():
    # occ - begin < rt2 at residues 1..3 (a domain may begin at each): start follows; at 4 it stays
    occ = np.array([0.05, 0.2, 0.6, 0.9, 0.9, 0.05], np.float32)
    begin = np.array([0.0, 0.15, 0.55, 0.1, 0.0, 0.0], np.float32)
    end = np.zeros(6, np.float32)
    assert regions(begin, end, occ) == [(3, 6)]
    # without the begin mass the start stays at the first residue scanned
    assert regions(np.zeros(6, np.float32), end, np.array([0.2, 0.2, 0.6, 0.9, 0.9, 0.05], np.float32)) == [(1, 6)]


# ---- scan constants, struct layout, sanitizers -------------------------------------------------------------------

SCAN_CASES = [(1, 2), (65, 2), (128, 2), (300, 6), (1400, 22), (1407, 22), (2432, 38)]
# the sparse-lane lengths of every S, each once ((65, 2) is above already; 385 is two of S = 12's three)
SCAN_CASES += [c for c in dict.fromkeys((leng, S) for S in SLOTS for leng in sparse_lengths(S)) if c not in SCAN_CASES]


@pytest.mark.parametrize("leng,S", SCAN_CASES)
def test_scan_constants_against_reversed_cumprod(leng, S):
    rng = np.random.Generator(np.random.PCG64(leng))
    M = leng + 1
    tsc = np.log(rng.uniform(0.05, 1.0, (M, 7))).astype(np.float32)
    dd, suffix, steps = np.zeros((64, S), np.float32), np.zeros((64, S), np.float32), np.zeros((6, 64), np.float32)
    assert _native.lib().msv_dom_scan_constants(tsc.ctypes.data, M, S, dd.ctypes.data, suffix.ctypes.data,
                                                steps.ctypes.data) == 0
    # slot q of lane l is state k = l S + q + 1; the d->d OUT of it is node k's own, for k = 1 .. LENG-1
    want_dd = np.zeros(64 * S)
    k = np.arange(1, 64 * S + 1)
    real = (k >= 1) & (k <= leng - 1)
    want_dd[real] = np.exp(tsc[k[real], DD].astype(np.float64))
    assert np.array_equal(dd.ravel(), want_dd.astype(np.float32))
    lanes = dd.astype(np.float64)
    rev = np.cumprod(lanes[:, ::-1], axis=1)[:, ::-1]
    np.testing.assert_allclose(suffix, rev, rtol=2.0 ** -23, atol=1e-45)
    whole = rev[:, 0]
    for j in range(6):
        want = np.array([np.prod(whole[l:min(64, l + 2 ** j)]) for l in range(64)])
        np.testing.assert_allclose(steps[j], want, rtol=2.0 ** -23, atol=1e-45)
    # padding: the suffix product of every slot beyond LENG (and of node LENG, which has no d->d), and A_j[l] of every
    # window l .. min(63, l + 2^j - 1) that reaches a padding lane (the lanes from LENG // S on), are exactly 0.0
    assert not suffix.ravel()[leng - 1:].any()
    for j in range(6 if leng < 64 * S else 0):
        assert not steps[j, max(0, leng // S - 2 ** j + 1):].any(), j
    assert _native.lib().msv_dom_scan_constants(tsc.ctypes.data, M, 3, None, None, None) == 1  # odd S
    if leng > 128:
        assert _native.lib().msv_dom_scan_constants(tsc.ctypes.data, M, 2, None, None, None) == 1  # S too small


def test_workspace_bytes_are_a_pure_function_of_the_length():
    L = _native.lib()
    assert [L.msv_dom_sequence_bytes(x) for x in (0, 1, 64, 131071)] == [24, 48, 24 * 65, 24 * 131072]


@pytest.mark.parametrize("struct,py", [("msv_dom_info", _native.DomInfo), ("msv_dom_stats", _native.DomStats)])
def test_struct_layouts_match_the_header(tmp_path, struct, py):
    """The ctypes mirrors have the C header's field offsets and sizes (gcc on include/msv.h); msv_dom_info begins
    with struct_size, and msv_dom_region is REGION_DTYPE."""
    import subprocess
    src = ['#include <stddef.h>', '#include <stdio.h>', '#include "msv.h"', "int main(void) {",
           f'  printf("size %zu\\n", sizeof({struct}));', '  printf("region %zu\\n", sizeof(msv_dom_region));']
    src += [f'  printf("{f} %zu\\n", offsetof({struct}, {f}));' for f, _ in py._fields_]
    src += [f'  printf("r_{f} %zu\\n", offsetof(msv_dom_region, {f}));' for f, _ in _native.REGION_DTYPE]
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
    dt = np.dtype(_native.REGION_DTYPE)
    assert int(got["region"]) == dt.itemsize
    for f, _ in _native.REGION_DTYPE:
        assert int(got[f"r_{f}"]) == dt.fields[f][1], f
    if struct == "msv_dom_info":
        assert py._fields_[0][0] == "struct_size" and int(got["struct_size"]) == 0


def test_asan_decode():
    """tests/cpp/sanitize_decode.cpp under AddressSanitizer + UBSan: the CPU decode, the rule, the Backward table
    builders at exact fit and the workspace arithmetic, a stand-alone program built from the host-only sources (no
    code loaded into Python is run under a sanitizer)."""
    import subprocess
    p = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "hmm_fasta_viterbi_amd", "csrc"), "asan_decode"],
                       capture_output=True, text=True, timeout=900)
    out = p.stdout + p.stderr
    assert p.returncode == 0, out[-4000:]
    assert "sanitize_decode passed" in out
    assert "ERROR: AddressSanitizer" not in out and "runtime error:" not in out
