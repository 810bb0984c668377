"""The domain stage's CPU reference (msv_dom_cpu_decode, float64) against an INDEPENDENT FORMULATION: every state
path of test_forward_paths.py's enumeration, here with each path recording the rows at which it passes B, the rows at
which it passes E and the residues its core states (M, I) emit.  No dynamic programming, no matrices:
    Backward score = log of the summed path odds (path_sum, imported)
    begin[i] = the share of the paths' odds that passes B at row i - 1 (its next state is an M that emits residue i)
    end[i]   = the share that passes E at row i (the domain's last emitted residue is i)
    occ[i]   = the share whose core emits residue i
This pins what the Backward recurrence cannot pin against itself: the silent D chain of row L, the exits entering
every D with k >= 2 (not D_1), which node's transition each step reads, and the order of the specials."""
import math

import numpy as np
import pytest

import hmm_fasta_viterbi_amd as msv
from decode_lib import cpu_decode, np_decode
from forward_lib import MM, MI, MD, IM, II, DM, DD
from test_forward_paths import path_sum
from test_viterbi_paths import random_model


def path_posteriors(msc, isc, tsc, consts, codes):
    """(log Z, begin, end, occ) from the explicit enumeration; begin / end / occ float64 [L]."""
    tBM, tEC, tEJ = (float(x) for x in consts)
    leng = msc.shape[1] - 1
    L = len(codes)
    loop, move = (float(x) for x in msv.sequence_transitions(L))
    t = tsc.astype(np.float64)
    paths = []  # (score, B rows as bits of residue i = row + 1, E rows as bits, core-emitted residues as bits)

    def em(k, pos):
        return float(msc[codes[pos - 1], k])

    def ei(k, pos):
        return 0.0 if isc is None else float(isc[codes[pos - 1], k])

    def m_state(pos, k, s, b, e, o):
        s = s + em(k, pos)
        o = o | (1 << pos)
        e_state(pos, s, b, e, o)
        if k < leng:
            if pos < L:
                m_state(pos + 1, k + 1, s + t[k, MM], b, e, o)
                i_state(pos + 1, k, s + t[k, MI], b, e, o)
            d_state(pos, k + 1, s + t[k, MD], b, e, o)

    def i_state(pos, k, s, b, e, o):
        s = s + ei(k, pos)
        o = o | (1 << pos)
        if pos < L:
            i_state(pos + 1, k, s + t[k, II], b, e, o)
            m_state(pos + 1, k + 1, s + t[k, IM], b, e, o)

    def d_state(pos, k, s, b, e, o):
        e_state(pos, s, b, e, o)
        if k < leng:
            d_state(pos, k + 1, s + t[k, DD], b, e, o)
            if pos < L:
                m_state(pos + 1, k + 1, s + t[k, DM], b, e, o)

    def enter(pos, s, b, e, o):      # B at row pos: the next state is an M that emits residue pos + 1
        if pos < L:
            b = b | (1 << (pos + 1))
            for k in range(1, leng + 1):
                m_state(pos + 1, k, s + tBM, b, e, o)

    def e_state(pos, s, b, e, o):    # E at row pos
        e = e | (1 << pos)
        paths.append((s + tEC + (L - pos) * loop + move, b, e, o))
        j = s + tEJ
        for m in range(0, L - pos):
            enter(pos + m, j + move, b, e, o)
            j = j + loop

    n = 0.0
    for pos in range(0, L):
        enter(pos, n + move, 0, 0, 0)
        n = n + loop
    score = np.array([p[0] for p in paths])
    marks = np.array([p[1:] for p in paths], np.int64)  # [paths][3]
    top = score.max()
    w = np.exp(score - top)  # (-inf: 0)
    z = w.sum()  # (numpy's pairwise sum: 1e5 non-negative terms to 1e-15)
    out = [np.array([w[(marks[:, field] >> i) & 1 == 1].sum() / z for i in range(1, L + 1)]) for field in range(3)]
    return (top + math.log(z), *out)


def _cases(leng, inserts):
    rng = np.random.Generator(np.random.PCG64(4000 * leng + inserts))
    for trial in range(4 if leng < 5 else 2):
        msc, isc, tsc, consts = random_model(rng, leng, inserts)
        if trial % 2:  # distinct exits: C and J no longer coincide
            consts = (consts[0], np.float32(consts[1] - np.float32(0.75)), consts[2])
        for L in (0, 1, 2, 3, 4, 5):
            yield trial, L, (msc, isc, tsc, consts), rng.integers(0, 20, L, dtype=np.uint8)


@pytest.mark.parametrize("leng", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("inserts", [False, True])
def test_cpu_decode_equals_the_sums_over_explicit_paths(leng, inserts):
    for trial, L, model, codes in _cases(leng, inserts):
        st, fwd, bck, begin, end, occ = cpu_decode(*model, codes)
        assert st == 0
        if L == 0:
            assert fwd == -math.inf and bck == -math.inf
            continue
        want = path_sum(*model, codes)
        assert abs(bck - want) <= 1e-10 * abs(want), (leng, inserts, trial, L, bck, want)
        assert abs(fwd - want) <= 1e-10 * abs(want), (leng, inserts, trial, L, fwd, want)
        z, pb, pe, po = path_posteriors(*model, codes)
        assert abs(z - want) <= 1e-10 * abs(want)
        for name, got, ref in (("begin", begin, pb), ("end", end, pe), ("occ", occ, po)):
            assert np.all(np.abs(got - ref) <= 1e-10), (leng, inserts, trial, L, name, got, ref)


def test_the_numpy_restatement_agrees_and_the_row_L_chain_carries_weight():
    """Not vacuous: a Backward that leaves the silent D chain out of row L (bM(L,k) = bE(L), no m->d .. d->d exits
    after the last residue) fails the same comparison visibly, on the begin posteriors and on the Backward score."""
    rng = np.random.Generator(np.random.PCG64(77))
    seen = 0.0
    for trial in range(4):
        model = random_model(rng, 4, False)
        codes = rng.integers(0, 20, 4, dtype=np.uint8)
        z, pb, pe, po = path_posteriors(*model, codes)
        good = np_decode(*model, codes)
        assert abs(good["bck"] - z) <= 1e-10 * abs(z) and abs(good["fwd"] - z) <= 1e-10 * abs(z)
        for name, ref in (("begin", pb), ("end", pe), ("occ", po), ("occ_core", po)):
            assert np.all(np.abs(good[name] - ref) <= 1e-10), (trial, name)
        cut = np_decode(*model, codes, row_L_chain=False)
        seen = max(seen, float(np.abs(cut["begin"] - pb).max()), abs(cut["bck"] - z))
    print(f"row-L chain left out: posteriors or score move by up to {seen:.3e}")
    assert seen > 1e-6
