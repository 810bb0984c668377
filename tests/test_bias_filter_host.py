"""The bias filter's host half (bias_filter_host.cpp, msv.h "Bias filter") without a GPU: the parser's
COMPO values, the float64 definition against an explicit sum over every state path and against closed forms, its
robustness, the filtered P-value arithmetic against msv_pvalues / msv_fwd_pvalues (bitwise at zero bias) and a float64
restatement, the device table, and the premise of the GPU cascade test on the float64 twin."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

from hmm_fasta_viterbi_amd import _native
import hmm_fasta_viterbi_amd as msv

import bias_filter_lib as bfl
from bias_filter_lib import EXPONENTIAL, GUMBEL, background, cpu_score, odds, pvalues
from oracle_lib import ROOT

PROFILES = sorted(glob.glob(os.path.join(ROOT, "data", "profile_HMMs", "*.hmm")))


# ---- parser ---------------------------------------------------------------------------------------------------------

def test_every_bundled_profile_is_covered():
    assert len(PROFILES) == 24


@pytest.mark.parametrize("path", PROFILES, ids=[os.path.basename(p) for p in PROFILES])
def test_compo_is_the_files_compo_line(path):
    h = msv.Profile_HMM(path)
    want = bfl.numpy_compo(path)
    assert h.compo.dtype == np.float32 and h.compo.shape == (20,)
    assert np.array_equal(h.compo.view(np.uint32), want.view(np.uint32))
    assert abs(float(h.compo.astype(np.float64).sum()) - 1.0) < 1e-5


def test_background_is_the_librarys():
    """The accessor returns the table the MSV precompute divides by: log(match / background) reproduces msv_scores."""
    h = msv.Profile_HMM(PROFILES[0])
    es, *_ = h.msv_scores()
    bg = background()
    assert bg.dtype == np.float32 and abs(float(bg.astype(np.float64).sum()) - 1.0) < 1e-5
    with np.errstate(divide="ignore"):
        want = np.log(h.match_emissions / bg[None, :]).T.astype(np.float32)
    assert np.allclose(es[:, 1:], want[:, 1:], rtol=1e-6, atol=1e-6)


# ---- the definition -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("leng", [1, 7, 8, 100, 2405])
def test_definition_is_the_sum_over_every_state_path(leng):
    rng = np.random.Generator(np.random.PCG64(leng))
    bg = background()
    compo = bfl.file_compo("100")[0] if leng == 100 else bfl.file_compo("2405")[0] if leng == 2405 else \
        bfl.synthetic_compo(leng, 0.2, 5.0)
    for L in range(1, 11):
        codes = rng.integers(0, 20, L).astype(np.uint8)
        st, got = cpu_score(compo, bg, leng + 1, codes)
        assert st == 0
        assert abs(got - bfl.path_sum(compo, bg, leng + 1, codes)) <= 1e-12, (leng, L)


@pytest.mark.parametrize("L", [1, 500, 20000])
def test_a_composition_equal_to_the_background_scores_zero(L):
    bg = background()
    codes = np.random.Generator(np.random.PCG64(L)).integers(0, 20, L).astype(np.uint8)
    for leng in (1, 100, 2405):
        st, got = cpu_score(bg, bg, leng + 1, codes)
        assert st == 0 and abs(got) <= 1e-12


@pytest.mark.parametrize("name", ["100", "1400", "2405"])
def test_homopolymer_lower_bound(name):
    """The path that starts in the biased state and stays there is one term of the non-negative sum."""
    compo, M = bfl.file_compo(name)
    bg = background()
    r = odds(compo, bg)
    a = int(np.argmax(r))
    T, pi = bfl.transitions(M)
    for L in (1, 17, 400, 5000):
        st, got = cpu_score(compo, bg, M, np.full(L, a, np.uint8))
        bound = np.log(pi[1]) + (L - 1) * np.log(T[1, 1]) + L * np.log(r[a])
        assert st == 0 and got >= bound - 1e-9 * abs(bound)
    # (and a long one is far above a background sequence's few nats)
    assert got > 50.0


def test_empty_sequence_scores_zero():
    compo, M = bfl.file_compo("100")
    assert cpu_score(compo, background(), M, np.zeros(0, np.uint8)) == (0, 0.0)
    st, out = bfl.cpu_score_batch(compo, background(), M, np.array([3, 4], np.uint8), np.array([0, 0, 2, 2], np.uint64))
    assert st == 0 and out[0] == 0.0 and out[2] == 0.0 and out[1] == cpu_score(compo, background(), M, [3, 4])[1]


def test_background_sequences_score_a_few_nats():
    compo, M = bfl.file_compo("100")
    codes, offsets = bfl.cascade_batch()
    st, out = bfl.cpu_score_batch(compo, background(), M, codes, offsets)
    assert st == 0 and out[:bfl.N_BACKGROUND].min() > -0.8 and out[:bfl.N_BACKGROUND].max() < 2.8


# ---- robustness -----------------------------------------------------------------------------------------------------

def test_bad_code_is_refused():
    compo, M = bfl.file_compo("100")
    codes = np.array([0, 1, 20, 3], np.uint8)
    assert cpu_score(compo, background(), M, codes)[0] == _native.MSV_ERR_BAD_RESIDUE
    st, _ = bfl.cpu_score_batch(compo, background(), M, codes, np.array([0, 2, 4], np.uint64))
    assert st == _native.MSV_ERR_BAD_RESIDUE


def test_extreme_composition_stays_finite():
    bg = background()
    compo = bfl.synthetic_compo(12, 0.05, 20.0)
    r = odds(compo, bg)
    assert r.max() / r.min() > 300.0
    hi, lo = int(np.argmax(r)), int(np.argmin(r))
    L = 50000
    alt = np.where(np.arange(L) % 2 == 0, hi, lo).astype(np.uint8)
    for leng in (1, 300):
        for codes in (np.full(L, hi, np.uint8), np.full(L, lo, np.uint8), alt):
            st, got = cpu_score(compo, bg, leng + 1, codes)
            assert st == 0 and np.isfinite(got)
    # the largest-odds homopolymer's score is about L log r; the smallest's is the path that stays in the
    # background state, pi0 t00^(L-1), and little more
    assert cpu_score(compo, bg, 301, np.full(L, hi, np.uint8))[1] > 0.9 * L * np.log(r[hi])
    T, pi = bfl.transitions(301)
    stay = np.log(pi[0]) + (L - 1) * np.log(T[0, 0])
    assert stay <= cpu_score(compo, bg, 301, np.full(L, lo, np.uint8))[1] < stay + 1.0


def test_device_table_is_the_rounded_model():
    compo, M = bfl.file_compo("2405")
    bg = background()
    table = np.zeros(26, np.float32)
    assert _native.lib().msv_bf_device_table(compo.ctypes.data, bg.ctypes.data, M, table.ctypes.data) == 0
    T, pi = bfl.transitions(M)
    want = np.concatenate([T.ravel(), pi, odds(compo, bg)]).astype(np.float32)
    assert np.array_equal(table.view(np.uint32), want.view(np.uint32))
    # odds outside [2^-24, 2^7] are refused for the float32 kernel (the definition takes them)
    wild = compo.copy()
    wild[3] = 50.0
    assert _native.lib().msv_bf_device_table(wild.ctypes.data, bg.ctypes.data, M, table.ctypes.data) == 6
    assert cpu_score(wild, bg, M, np.array([3, 3], np.uint8))[0] == 0


# ---- the filtered P-values ------------------------------------------------------------------------------------------

def _random_scores(seed, n):
    rng = np.random.Generator(np.random.PCG64(seed))
    lengths = rng.integers(0, 3000, n)
    lengths[:3] = 0, 1, 2
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
    scores = rng.normal(-2.0, 6.0, n).astype(np.float32)
    scores[3:6] = -np.inf, 120.0, -300.0
    return scores, offsets, rng


@pytest.mark.parametrize("kind,fn", [(GUMBEL, "msv_pvalues"), (EXPONENTIAL, "msv_fwd_pvalues")])
def test_zero_bias_is_the_unfiltered_pvalue_bitwise(kind, fn):
    scores, offsets, _ = _random_scores(1, 4000)
    want = np.zeros(len(scores))
    for loc, scale in ((-8.6, 0.71), (-3.2, 0.69), (1.5, 0.3)):
        assert getattr(_native.lib(), fn)(scores.ctypes.data, offsets.ctypes.data, len(scores), loc, scale,
                                          want.ctypes.data) == 0
        for zero in (0.0, -0.0):
            st, got = pvalues(scores, np.full(len(scores), zero, np.float32), offsets, loc, scale, kind)
            assert st == 0 and np.array_equal(got.view(np.uint64), want.view(np.uint64))


@pytest.mark.parametrize("kind", [GUMBEL, EXPONENTIAL])
def test_pvalues_with_bias_match_float64_and_are_monotone(kind):
    scores, offsets, rng = _random_scores(2, 3000)
    bias = rng.uniform(-1.0, 30.0, len(scores)).astype(np.float32)
    loc, scale = -8.6, 0.71
    st, got = pvalues(scores, bias, offsets, loc, scale, kind)
    assert st == 0
    lengths = np.diff(offsets).astype(np.int64)
    want = np.array([bfl.pvalue64(s, b, int(L), np.float32(loc), np.float32(scale), kind)
                     for s, b, L in zip(scores, bias, lengths)])
    # the float32 bits carry |bits| 2^-23 or so into the exponent: relative 1e-6 on P wherever P is not denormal
    ok = want > 1e-290
    assert np.all(np.abs(got[ok] - want[ok]) <= 1e-6 * want[ok] + 1e-300)
    # a larger bias never lowers P
    st, more = pvalues(scores, bias + np.float32(0.75), offsets, loc, scale, kind)
    assert st == 0 and np.all(more >= got)
    # a score of -inf gives 1 whatever the bias; so does an empty sequence
    ninf = np.full(len(scores), -np.inf, np.float32)
    for b in (bias, np.full(len(scores), np.inf, np.float32)):
        st, one = pvalues(ninf, b, offsets, loc, scale, kind)
        assert st == 0 and np.all(one == 1.0)
    assert got[0] == 1.0


def test_pvalues_refuse_bad_arguments():
    scores, offsets, _ = _random_scores(3, 8)
    zero = np.zeros(8, np.float32)
    assert pvalues(scores, zero, offsets, 0.0, 1.0, 2)[0] == 1
    bad = offsets.copy()
    bad[4] = bad[3] - 1
    assert pvalues(scores, zero, bad, 0.0, 1.0, GUMBEL)[0] == 1
    assert _native.lib().msv_bf_pvalues(None, None, None, 0, 0.0, 1.0, GUMBEL, None) == 0


# ---- the GPU cascade test's premise ---------------------------------------------------------------------------------

def test_cascade_batch_has_a_planted_sequence_only_the_filter_removes():
    """On the float64 twin and the bit-exact CPU MSV score: a planted sequence passes P <= F1 against null1 and fails
    it against the filtered score, each with a margin of 1 bit."""
    msc, bias, bits1, bits2, cut = bfl.cascade_reference()
    planted = np.arange(bfl.N_BACKGROUND, bfl.N_BACKGROUND + bfl.N_PLANTED)
    removed = planted[(bits1[planted] >= cut + 1.0) & (bits2[planted] <= cut - 1.0)]
    assert removed.size >= 1
    # and the P-values the library gives say the same
    o = bfl.OracleProfile("100")
    mu, lam = float(o.stats()[0]), float(o.stats()[1])
    _, offsets = bfl.cascade_batch()
    _, p1 = pvalues(msc, np.zeros(len(msc), np.float32), offsets, mu, lam, GUMBEL)
    _, p2 = pvalues(msc, bias.astype(np.float32), offsets, mu, lam, GUMBEL)
    assert np.all(p1[removed] <= 0.02) and np.all(p2[removed] > 0.02)
