"""The bias stage's host half (msv.h "Bias stage"; csrc/null2_host.cpp): msv_aln_cpu_null2 against an
explicit enumeration of every state path of tiny models, the two properties the model implies, the definition of the
correction, the bias / bit score / P-value arithmetic against a restatement, the input condition of the domcorrection
bound on every item of the GPU tests' lists, the struct layouts and the stand-alone sanitizer program."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import hmm_fasta_viterbi_amd as msv
from hmm_fasta_viterbi_amd import _native
from align_lib import cpu_decode
from forward_batches import base_model
from null2_lib import (OMEGA, bias_scores, case, condition_holds, correction, cpu_null2, enumerated_null2,
                       null2_bound)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LN2F = np.float32(0.69314718055994529)


def _codes(Le, seed):
    return np.random.Generator(np.random.PCG64(seed)).integers(0, 20, size=Le, dtype=np.uint8)


def _definition64(null2, codes):
    n = np.bincount(codes.astype(np.int64), minlength=20)
    return float(sum(n[x] * np.log(null2[x]) for x in range(20) if n[x]))


@pytest.mark.parametrize("inserts", (False, True))
@pytest.mark.parametrize("leng", (1, 2, 3, 4))
def test_null2_against_every_path_of_tiny_models(leng, inserts):
    model = base_model(leng, 5100 + leng, inserts)
    for Le in (1, 2, 3, 4):
        for rep in range(2):
            codes = _codes(Le, 89 * leng + 13 * Le + rep)
            for Lc in (Le, Le + 7):
                st, n2, dc = cpu_null2(model, codes, Lc)
                assert st == 0
                want = enumerated_null2(model, codes, Lc)
                assert np.max(np.abs(n2 - want)) <= 1e-10, (leng, Le, Lc)
                assert abs(dc - _definition64(want, codes)) <= 1e-9


def test_zero_score_model_has_null2_one():
    """Every emission score 0: rows of posteriors sum to 1, so null2 = 1 and the correction is 0."""
    for leng, inserts in ((1, False), (3, True), (70, False), (129, True)):
        msc, isc, tsc, consts = base_model(leng, 5200 + leng, inserts)
        msc = np.zeros_like(msc)
        msc[:, 0] = -np.inf
        model = (msc, None if isc is None else np.zeros_like(isc), tsc, consts)
        for Le, Lc in ((1, 1), (5, 5), (40, 90), (90, 390)):
            st, n2, dc = cpu_null2(model, _codes(Le, 7 * leng + Le), Lc)
            assert st == 0
            assert np.max(np.abs(n2 - 1.0)) <= 1e-12 and abs(dc) <= 1e-12


def test_biased_model_is_corrected_downwards():
    """Every match state gives residue a odds >= c > 1, insert odds 1, the envelope made of a only: null2[a] >=
    1 + (c - 1) sum_k eM(k) / Le > 1, the correction is positive and the corrected bits are below the uncorrected."""
    a, c = 7, 2.5
    for leng in (3, 40):
        msc, _, tsc, consts = base_model(leng, 5300 + leng, False)
        rng = np.random.Generator(np.random.PCG64(leng))
        msc = msc.copy()
        msc[a, 1:] = np.log(c + rng.uniform(0.0, 2.0, leng)).astype(np.float32)
        model = (msc, None, tsc, consts)
        for Le, Lc in ((4, 4), (30, 30), (30, 200)):
            codes = np.full(Le, a, np.uint8)
            st, n2, dc = cpu_null2(model, codes, Lc)
            assert st == 0
            _, _, pm, *_ = cpu_decode(model, codes, Lc)
            c32 = float(np.exp(np.float64(msc[a, 1:])).astype(np.float32).min())
            floor = 1.0 + (c32 - 1.0) * pm.sum() / Le
            assert pm.sum() > 0 and n2[a] >= floor * (1 - 1e-12) and n2[a] > 1.0
            assert dc > 0.0 and abs(dc - Le * np.log(n2[a])) <= 1e-12 * abs(dc)
            env = np.array([3.0], np.float32)
            st, with_bias = bias_scores(env, [Le], [Lc], [dc], -3.0, 0.7)
            st2, without = bias_scores(env, [Le], [Lc], [-np.inf], -3.0, 0.7)
            assert st == 0 and st2 == 0 and without["dombias"][0] == 0.0
            assert with_bias["domain_bits"][0] < without["domain_bits"][0]


def test_the_definition_of_the_correction():
    # by hand: residues 3, 3, 5 with null2[3] = 2, null2[5] = 1/2 -> 2 log 2 + log(1/2) = log 2
    v = np.ones(20, np.float32)
    v[3], v[5] = 2.0, 0.5
    st, dc = correction(v, [3, 3, 5])
    assert st == 0 and dc == np.float32(np.log(2.0))
    # n_x = 0 terms are skipped: a zero, a negative number, an infinity and a NaN where no residue points
    w = v.copy()
    w[0], w[1], w[2], w[19] = 0.0, -1.0, np.inf, np.nan
    assert correction(w, [3, 3, 5]) == (0, dc)
    # the order is x = 0 .. 19 in float64 with ONE rounding: terms whose float64 sum depends on the order
    rng = np.random.Generator(np.random.PCG64(9))
    for _ in range(50):
        n2 = np.exp(rng.normal(0.0, 2.0, 20)).astype(np.float32)
        codes = rng.integers(0, 20, int(rng.integers(1, 400)), dtype=np.uint8)
        n = np.bincount(codes.astype(np.int64), minlength=20)
        acc = np.float64(0.0)
        for x in range(20):
            if n[x]:
                acc = acc + np.float64(n[x]) * np.log(np.float64(n2[x]))
        st, got = correction(n2, codes)
        assert st == 0 and got == np.float32(acc)
    assert correction(v, [])[1] == 0.0 and correction(v, [20])[0] == 4
    assert _native.lib().msv_aln_null2_correction(None, None, 0, None) == 1


def test_cpu_null2_argument_classes():
    model = base_model(5, 5400, True)
    assert cpu_null2(model, [1, 2, 20])[0] == 4
    assert cpu_null2(model, [1, 2, 3], Lc=2)[0] == 1
    assert cpu_null2(model, [])[0] == 1
    L = _native.lib()
    from forward_lib import _args
    c = np.array([1, 2, 3], np.uint8)
    dc = C.c_double()
    assert L.msv_aln_cpu_null2(*_args(*model), c.ctypes.data, 3, 3, None, C.byref(dc)) == 0  # null2 may be NULL
    assert L.msv_aln_cpu_null2(*_args(*model), c.ctypes.data, 3, 3, None, None) == 0
    assert dc.value == cpu_null2(model, c)[2]


def test_bias_scores_against_a_restatement():
    """The formulas of msv.h written out: float32 where msv_fwd_pvalues is float32 (its own test's roundings), the logs
    and the sums of corrections in float64 rounded once; and against plain float64 within float32 roundings."""
    rng = np.random.Generator(np.random.PCG64(41))
    n_seq, m = 9, 40
    lengths = rng.integers(1, 3000, n_seq)
    lengths[0] = 0
    parent = rng.integers(1, n_seq - 1, m)  # sequence 0 (empty) and the last have no item
    Lc = lengths[parent]
    Le = np.array([int(rng.integers(1, x + 1)) for x in Lc])
    Le[:3] = Lc[:3]
    env = rng.normal(20.0, 30.0, m).astype(np.float32)
    dc = rng.normal(0.0, 6.0, m).astype(np.float32)
    dc[5], env[6] = 0.0, np.inf
    fwd = rng.normal(25.0, 30.0, n_seq).astype(np.float32)
    fwd[0] = -np.inf
    tau, lam = np.float32(-4.1234), np.float32(0.71)
    st, out = bias_scores(env, Le, Lc, dc, tau, lam, parent, fwd, lengths)
    assert st == 0

    def nullsc(L):
        p1 = np.float32(L) / np.float32(L + 1)
        return np.float32(L * np.log(np.float64(p1)) + np.log(1.0 - np.float64(p1)))

    def tail(bits):
        return 1.0 if bits < tau else np.exp(-np.float64(lam) * (np.float64(bits) - np.float64(tau)))

    with np.errstate(invalid="ignore", over="ignore"):
        for q in range(m):
            bias = np.float32(np.log(1.0 + OMEGA * np.exp(np.float64(dc[q]))))
            loop = np.float32(msv.sequence_transitions(int(Lc[q]))[0])
            dom = np.float32(env[q] + np.float32((np.float32(Lc[q]) - np.float32(Le[q])) * loop))
            bits = np.float32(np.float32(np.float32(dom - nullsc(int(Lc[q]))) - bias) / LN2F)
            assert out["dombias"][q] == bias and out["domain_bits"][q] == bits, q
            assert out["domain_pvalues"][q] == pytest.approx(tail(bits), rel=1e-12, abs=0.0)
            # plain float64
            want = (np.float64(env[q]) + (int(Lc[q]) - int(Le[q])) * np.log(int(Lc[q]) / (int(Lc[q]) + 3.0))
                    - np.float64(nullsc(int(Lc[q])))  # (null1's p1 is a float32, as p7_bg_NullOne's)
                    - np.log1p(OMEGA * np.exp(np.float64(dc[q])))) / np.log(2.0)
            if np.isfinite(want):
                # the loop score is the float32 log of a float32 ratio near 1: 2^-24 absolute per flank residue
                scale = abs(float(env[q])) + 2 * (int(Lc[q]) - int(Le[q])) + 30.0
                assert abs(float(out["domain_bits"][q]) - want) <= 8 * 2.0 ** -24 * scale / np.log(2.0), q
        assert out["domain_bits"][6] == np.inf and out["domain_pvalues"][6] == 0.0
        for s in range(n_seq):
            total = np.float64(0.0)
            for q in range(m):
                if parent[q] == s:
                    total = total + np.float64(dc[q])
            bias = np.float32(np.log(1.0 + OMEGA * np.exp(total)))
            assert out["seq_bias"][s] == bias, s
            if lengths[s] == 0:
                assert out["seq_bits"][s] == -np.inf and out["seq_pvalues"][s] == 1.0
                continue
            bits = np.float32(np.float32(np.float32(fwd[s] - nullsc(int(lengths[s]))) - bias) / LN2F)
            assert out["seq_bits"][s] == bits
            assert out["seq_pvalues"][s] == pytest.approx(tail(bits), rel=1e-12, abs=0.0)
        assert out["seq_bias"][n_seq - 1] == np.float32(np.log(1.0 + OMEGA))  # no item: log(1 + omega)
    # without sequences nothing per sequence is read; wrong arguments are refused
    st, alone = bias_scores(env, Le, Lc, dc, tau, lam)
    assert st == 0 and alone["domain_bits"].tobytes() == out["domain_bits"].tobytes()
    assert bias_scores(env[:1], [3], [2], dc[:1], tau, lam)[0] == 1
    assert bias_scores(env[:1], [0], [2], dc[:1], tau, lam)[0] == 1
    assert bias_scores(env[:1], [1], [2], dc[:1], tau, lam, [1], fwd[:1], lengths[:1])[0] == 1


def test_sequence_transitions_loop_is_what_the_restatement_assumes():
    for L in (1, 7, 400):
        assert msv.sequence_transitions(L)[0] == pytest.approx(np.log(L / (L + 3.0)), rel=0.0, abs=4 * 2.0 ** -24)


@pytest.mark.parametrize("S,isc", [(2, False), (6, True), (12, False), (22, True), (38, False), (2, True), (6, False),
                                   (12, True), (22, False), (38, True)])
def test_input_condition_of_the_domcorrection_bound(S, isc):
    """delta_x <= null2_cpu[x] / 2 for every residue that occurs, on EVERY item of the GPU tests' lists (the bad item
    has no null2 and is compared with zeros there): a condition on the inputs, not a measurement."""
    worst = 0.0
    for which in range(3):
        model, codes, offsets, items, bad, refs = case(S, isc, which)
        off = offsets.astype(np.int64)
        assert len(items) >= 10 and bad == len(items) - 1
        for q, (s, a, b) in enumerate(items):
            if q == bad:
                continue
            n2, dc = refs[q]
            env = codes[off[s] + a - 1:off[s] + b]
            delta = null2_bound(model, b - a + 1, n2)
            occ = np.bincount(env.astype(np.int64), minlength=20) > 0
            worst = max(worst, float(np.max(delta[occ] / n2[occ])))
            assert condition_holds(env, n2, delta), (S, isc, which, q)
    print(f"S {S} isc {isc}: worst delta_x / null2_cpu[x] over occurring residues {worst:.3e} (must be <= 0.5)")


@pytest.mark.parametrize("struct,py", [("msv_aln_info", _native.AlnInfo), ("msv_aln_options", _native.AlnOptions),
                                       ("msv_aln_null2_stats", _native.AlnNull2Stats)])
def test_struct_layouts_match_the_header(tmp_path, struct, py):
    src = ['#include <stddef.h>', '#include <stdio.h>', '#include "msv.h"', "int main(void) {",
           f'  printf("size %zu\\n", sizeof({struct}));']
    src += [f'  printf("{f} %zu\\n", offsetof({struct}, {f}));' for f, _ in py._fields_]
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
    assert py._fields_[0][0] == "struct_size" and int(got["struct_size"]) == 0


def test_null2_host_sanitizer():
    """tests/cpp/sanitize_null2.cpp under AddressSanitizer + UBSan (csrc/Makefile `asan_null2`): a stand-alone program
    over the host-only sources; no code loaded into Python runs under a sanitizer."""
    p = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "hmm_fasta_viterbi_amd", "csrc"), "asan_null2"],
                       capture_output=True, text=True, timeout=900)
    out = p.stdout + p.stderr
    assert p.returncode == 0, out[-4000:]
    assert "sanitize_null2 passed" in out
    assert "ERROR: AddressSanitizer" not in out and "runtime error:" not in out
