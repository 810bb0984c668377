"""The Forward stage's CPU reference (msv_fwd_cpu_score, float64) against an INDEPENDENT FORMULATION of the model:
every state path through the multihit local model of test_viterbi_paths.py, enumerated explicitly on tiny models
and sequences -- here with the D_k -> E exits of HMMER3's p7_GForward added -- each path scored left to right in
float64, and the paths SUMMED: log sum exp(path).  No dynamic programming, no matrices.

This pins what the DP cannot pin against itself: which node's transition each step reads, that there is no I at
node LENG, that D_k (k >= 2) exits to E at no cost, that E is a sum over M and D, and the order of the specials
(N loops, B = (N + J) move, J / C loops, C(L) move)."""
import math

import numpy as np
import pytest

import hmm_fasta_viterbi_amd as msv
from forward_lib import MM, MI, MD, IM, II, DM, DD, cpu_score
from test_viterbi_paths import random_model


def path_sum(msc, isc, tsc, consts, codes, d_exits=True):
    """log of the sum over every state path of exp(its score), float64 (-inf when no path exists)."""
    tBM, tEC, tEJ = (float(x) for x in consts)
    leng = msc.shape[1] - 1
    L = len(codes)
    loop, move = (float(x) for x in msv.sequence_transitions(L))
    t = tsc.astype(np.float64)
    paths = []

    def em(k, pos):
        return float(msc[codes[pos - 1], k])

    def ei(k, pos):
        return 0.0 if isc is None else float(isc[codes[pos - 1], k])

    def m_state(pos, k, s):          # s: the score entering M_k (transition added); M_k emits residue pos
        s = s + em(k, pos)
        e_state(pos, s)              # local exit M_k -> E (no cost)
        if k < leng:                 # transitions out of node k exist for k = 1 .. LENG-1 only
            if pos < L:
                m_state(pos + 1, k + 1, s + t[k, MM])
                i_state(pos + 1, k, s + t[k, MI])
            d_state(pos, k + 1, s + t[k, MD])   # silent

    def i_state(pos, k, s):          # I_k (k <= LENG-1) emits residue pos
        s = s + ei(k, pos)
        if pos < L:
            i_state(pos + 1, k, s + t[k, II])
            m_state(pos + 1, k + 1, s + t[k, IM])

    def d_state(pos, k, s):          # D_k (k >= 2) at row pos, silent
        if d_exits:
            e_state(pos, s)          # local exit D_k -> E (no cost): p7_GForward's
        if k < leng:
            d_state(pos, k + 1, s + t[k, DD])
            if pos < L:
                m_state(pos + 1, k + 1, s + t[k, DM])

    def enter(pos, b):               # B at row pos -> M_k emits residue pos + 1
        if pos < L:
            for k in range(1, leng + 1):
                m_state(pos + 1, k, b + tBM)

    def e_state(pos, s):             # E at row pos
        paths.append(s + tEC + (L - pos) * loop + move)   # E -> C, C loops over the rest, then C(L) move
        j = s + tEJ                  # E -> J, J loops m times, then B -> another pass through the model
        for m in range(0, L - pos):
            enter(pos + m, j + move)
            j = j + loop

    n = 0.0                          # N(0) = 1; N loops, then B = N move
    for pos in range(0, L):
        enter(pos, n + move)
        n = n + loop
    finite = [p for p in paths if p > -math.inf]
    if not finite:
        return -math.inf
    top = max(finite)
    return top + math.log(math.fsum(math.exp(p - top) for p in finite))


@pytest.mark.parametrize("leng", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("inserts", [False, True])
def test_cpu_forward_equals_the_sum_over_explicit_paths(leng, inserts):
    rng = np.random.Generator(np.random.PCG64(2000 * leng + inserts))
    for trial in range(4 if leng < 5 else 2):  # (LENG 5 x L 5 enumerates ~10^5 paths per sequence)
        msc, isc, tsc, consts = random_model(rng, leng, inserts)
        if trial % 2:  # distinct exits: C and J no longer coincide
            consts = (consts[0], np.float32(consts[1] - np.float32(0.75)), consts[2])
        for L in (0, 1, 2, 3, 4, 5):
            codes = rng.integers(0, 20, L, dtype=np.uint8)
            want = path_sum(msc, isc, tsc, consts, codes)
            st, got = cpu_score(msc, isc, tsc, consts, codes)
            assert st == 0
            if L == 0:
                assert got == -math.inf and want == -math.inf
            else:
                assert abs(got - want) <= 1e-10 * abs(want), (leng, inserts, trial, L, got, want)


def test_the_enumeration_counts_the_d_exits():
    """Not vacuous: without the D -> E exits the path sum is visibly smaller on models with more than one node, so a
    DP that dropped them (as the Viterbi stage may) would fail the comparison above."""
    rng = np.random.Generator(np.random.PCG64(5))
    msc, isc, tsc, consts = random_model(rng, 4, False)
    codes = rng.integers(0, 20, 4, dtype=np.uint8)
    with_exits = path_sum(msc, isc, tsc, consts, codes)
    without = path_sum(msc, isc, tsc, consts, codes, d_exits=False)
    assert with_exits - without > 1e-4
    st, got = cpu_score(msc, isc, tsc, consts, codes)
    assert st == 0 and abs(got - with_exits) <= 1e-10 * abs(with_exits)
