"""Hand-built exact ties of the Viterbi trace, one builder per tie-break rule of msv.h ("Viterbi traces") (test
helper; host-only, not a conftest).  M takes M, I, D, B in that order (six pairwise rules); I takes M before I;
D takes M before D; E the smallest k; C and J the loop before E; B takes N before J: twelve rules.

Every case is a flat background model (every match score -3, every transition -2, entry -1) with a few planted
scores that put two paths far above the rest, and ONE free parameter solved so that the two predecessors of the
tied cell give the same float32 -- a few ulps around the real-number solution are tried.  The path enters from B
next to the anchor node `k` and the entry is uniform over nodes, so the solved parameter depends neither on k nor
on LENG.  The expected domains are written out from the construction and msv.h's order, never from an
implementation under test; `prove` shows without one that expected and alternative are two different legal paths
whose float32 re-scores both have the bits of the optimum."""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

import hmm_fasta_viterbi_amd as msv
from oracle_lib import bits
from trace_check import F, MM, MI, MD, IM, II, DM, DD, NINF, check_legal, rescore

NO_J = F(-50.0)  # tr_E_J that keeps J out of reach


class TieCase(NamedTuple):
    rule: str
    msc: np.ndarray
    isc: np.ndarray | None
    tsc: np.ndarray
    consts: tuple
    codes: np.ndarray
    expected: list      # the domains msv.h's order gives
    alternatives: list  # domain lists the other side(s) of the tie would give

    @property
    def tables(self):
        return self.msc, self.isc, self.tsc, self.consts


def flat_model(leng, e=-3.0):
    """Every match score `e`, transitions of a plain model, J out of reach (tr_E_J = -50), tr_E_C = -0.5."""
    M = leng + 1
    msc = np.full((20, M), F(e), F)
    msc[:, 0] = NINF
    tsc = np.full((M, 7), F(-2.0), F)
    return msc, tsc, (F(-1.0), F(-0.5), NO_J)


def insert_table(leng):
    """Informative insert scores: multiples of 1/8 in [-7/8, -1/8], never 0, different from node to node."""
    r, k = np.meshgrid(np.arange(20), np.arange(leng + 1), indexing="ij")
    return (-(1 + (3 * r + 5 * k) % 7) / 8.0).astype(F)


def solve(fn, target, x0):
    """A float32 x near x0 with fn(x) == target exactly (a few ulps around x0 are tried)."""
    lo = hi = F(x0)
    for _ in range(64):
        for x in (lo, hi):
            if fn(x) == target:
                return x
        lo, hi = np.nextafter(lo, F(-np.inf)), np.nextafter(hi, F(np.inf))
    raise AssertionError("no exact tie near x0")


def entry(L, tBM, i, B=None):
    """fl(B(i) + tBM) with B(i) = N(i) + move (N loops i times from 0), or with the given B."""
    loop, move = (F(x) for x in msv.sequence_transitions(L))
    if B is None:
        n = F(0.0)
        for _ in range(i):
            n = F(n + loop)
        B = F(n + move)
    return F(B + tBM)


def _start(leng, L, k, kmin, kmax, inserts=False):
    assert kmin <= k <= kmax, (k, kmin, kmax)
    msc, tsc, consts = flat_model(leng)
    return msc, (insert_table(leng) if inserts else None), tsc, consts, np.arange(L, dtype=np.uint8)


def _ins(isc, code, k):
    return F(0.0) if isc is None else isc[code, k]


# ---- the M cell: M(i,k) = max(M(i-1,k-1) + tMM, I(i-1,k-1) + tIM, D(i-1,k-1) + tDM, B(i-1) + tBM) + e, anchor k -----

def m_takes_m_before_i(leng, k, inserts=False):
    """a b c: B(1) -> M(2,k-1) -> M(3,k) against B(0) -> M(1,k-1) -> I(2,k-1) -> M(3,k); tIM solved."""
    msc, isc, tsc, consts, codes = _start(leng, 3, k, 2, leng, inserts)
    msc[0, k - 1], msc[1, k - 1], msc[2, k] = F(3.0), F(1.0), F(6.0)
    tsc[k - 1, MM] = F(-0.25)                    # (so that M(2,k-1) + tMM beats the entry from B(2))
    tBM = consts[0]
    i2 = F(F(F(entry(3, tBM, 0) + msc[0, k - 1]) + tsc[k - 1, MI]) + _ins(isc, 1, k - 1))
    cm = F(F(entry(3, tBM, 1) + msc[1, k - 1]) + tsc[k - 1, MM])
    tsc[k - 1, IM] = solve(lambda t: F(i2 + t), cm, F(cm - i2))
    assert tsc[k - 1, IM] <= 0
    return TieCase("M: M before I", msc, isc, tsc, consts, codes, [(2, 3, k - 1, k, b"MM")],
                   [[(1, 3, k - 1, k, b"MIM")]])


def m_takes_m_before_d(leng, k):
    """a b: B(0) -> M(1,k-1) -> M(2,k) against B(0) -> M(1,k-2) -> D(1,k-1) -> M(2,k); tDM solved."""
    msc, isc, tsc, consts, codes = _start(leng, 2, k, 3, leng)
    msc[0, k - 1], msc[0, k - 2], msc[1, k] = F(1.0), F(3.5), F(6.0)
    tsc[k - 1, MM] = F(-0.25)
    bt0 = entry(2, consts[0], 0)
    cm = F(F(bt0 + msc[0, k - 1]) + tsc[k - 1, MM])
    d = F(F(bt0 + msc[0, k - 2]) + tsc[k - 2, MD])
    tsc[k - 1, DM] = solve(lambda t: F(d + t), cm, F(cm - d))
    assert tsc[k - 1, DM] <= 0
    return TieCase("M: M before D", msc, isc, tsc, consts, codes, [(1, 2, k - 1, k, b"MM")],
                   [[(1, 2, k - 2, k, b"MDM")]])


def m_takes_m_before_b(leng, k):
    """a b: B(0) -> M(1,k-1) -> M(2,k) against B(1) -> M(2,k); tMM solved."""
    msc, isc, tsc, consts, codes = _start(leng, 2, k, 2, leng)
    msc[0, k - 1], msc[1, k] = F(1.0), F(5.0)
    m1 = F(entry(2, consts[0], 0) + msc[0, k - 1])
    bt1 = entry(2, consts[0], 1)
    tsc[k - 1, MM] = solve(lambda t: F(m1 + t), bt1, F(bt1 - m1))
    assert tsc[k - 1, MM] <= 0
    return TieCase("M: M before B", msc, isc, tsc, consts, codes, [(1, 2, k - 1, k, b"MM")], [[(2, 2, k, k, b"M")]])


def m_takes_i_before_d(leng, k, inserts=False):
    """a b c: B(0) -> M(1,k-1) -> I(2,k-1) -> M(3,k) against B(1) -> M(2,k-2) -> D(2,k-1) -> M(3,k); tDM solved."""
    msc, isc, tsc, consts, codes = _start(leng, 3, k, 3, leng, inserts)
    msc[0, k - 1], msc[1, k - 2], msc[2, k] = F(5.0), F(6.0), F(6.0)
    tBM = consts[0]
    i2 = F(F(F(entry(3, tBM, 0) + msc[0, k - 1]) + tsc[k - 1, MI]) + _ins(isc, 1, k - 1))
    ci = F(i2 + tsc[k - 1, IM])
    d = F(F(entry(3, tBM, 1) + msc[1, k - 2]) + tsc[k - 2, MD])
    tsc[k - 1, DM] = solve(lambda t: F(d + t), ci, F(ci - d))
    assert tsc[k - 1, DM] <= 0
    return TieCase("M: I before D", msc, isc, tsc, consts, codes, [(1, 3, k - 1, k, b"MIM")],
                   [[(2, 3, k - 2, k, b"MDM")]])


def m_takes_i_before_b(leng, k, inserts=False):
    """a b c: B(0) -> M(1,k-1) -> I(2,k-1) -> M(3,k) against B(2) -> M(3,k); tIM solved."""
    msc, isc, tsc, consts, codes = _start(leng, 3, k, 2, leng, inserts)
    msc[0, k - 1], msc[2, k] = F(5.0), F(6.0)
    tBM = consts[0]
    i2 = F(F(F(entry(3, tBM, 0) + msc[0, k - 1]) + tsc[k - 1, MI]) + _ins(isc, 1, k - 1))
    bt2 = entry(3, tBM, 2)
    tsc[k - 1, IM] = solve(lambda t: F(i2 + t), bt2, F(bt2 - i2))
    assert tsc[k - 1, IM] <= 0
    return TieCase("M: I before B", msc, isc, tsc, consts, codes, [(1, 3, k - 1, k, b"MIM")], [[(3, 3, k, k, b"M")]])


def m_takes_d_before_b(leng, k):
    """a b: B(0) -> M(1,k-2) -> D(1,k-1) -> M(2,k) against B(1) -> M(2,k); tDM solved."""
    msc, isc, tsc, consts, codes = _start(leng, 2, k, 3, leng)
    msc[0, k - 2], msc[1, k] = F(5.0), F(6.0)
    d = F(F(entry(2, consts[0], 0) + msc[0, k - 2]) + tsc[k - 2, MD])
    bt1 = entry(2, consts[0], 1)
    tsc[k - 1, DM] = solve(lambda t: F(d + t), bt1, F(bt1 - d))
    assert tsc[k - 1, DM] <= 0
    return TieCase("M: D before B", msc, isc, tsc, consts, codes, [(1, 2, k - 2, k, b"MDM")], [[(2, 2, k, k, b"M")]])


# ---- the I cell: I(i,k) = max(M(i-1,k) + tMI, I(i-1,k) + tII) (+ insert score), anchor k <= LENG - 1 ----------------

def i_takes_m_before_i(leng, k, inserts=False):
    """a b c d: B(1) -> M(2,k) -> I(3,k) -> M(4,k+1) against B(0) -> M(1,k) -> I(2,k) -> I(3,k) -> M(4,k+1); tII solved.
    With insert scores I(2,k) carries its own, and I(3,k)'s is added after the source is decided."""
    msc, isc, tsc, consts, codes = _start(leng, 4, k, 1, leng - 1, inserts)
    msc[0, k], msc[1, k], msc[3, k + 1] = F(9.0), F(6.0), F(8.0)
    tBM = consts[0]
    mi = F(F(entry(4, tBM, 1) + msc[1, k]) + tsc[k, MI])
    i2 = F(F(F(entry(4, tBM, 0) + msc[0, k]) + tsc[k, MI]) + _ins(isc, 1, k))
    tsc[k, II] = solve(lambda t: F(i2 + t), mi, F(mi - i2))
    assert tsc[k, II] <= 0
    return TieCase("I: M before I", msc, isc, tsc, consts, codes, [(2, 4, k, k + 1, b"MIM")],
                   [[(1, 4, k, k + 1, b"MIIM")]])


# ---- the D cell: D(i,k) = max(M(i,k-1) + tMD, D(i,k-1) + tDD), anchor k <= LENG - 1 (no D ends at the exit) ---------

def d_takes_m_before_d(leng, k, chain=1):
    """a b: B(0) -> M(1,k-1) -> D(1,k) -> M(2,k+1) against B(0) -> M(1,k-1-chain) -> D(1,k-chain) .. D(1,k) -> M(2,k+1),
    whose `chain` + 1 deletes run over d->d of -1/8 (exact sums) into the solved d->d of node k-1."""
    msc, isc, tsc, consts, codes = _start(leng, 2, k, chain + 2, leng - 1)
    first = k - 1 - chain
    msc[0, k - 1], msc[0, first], msc[1, k + 1] = F(5.0), F(6.0 + (chain - 1) / 8.0), F(8.0 + chain / 8.0)
    bt0 = entry(2, consts[0], 0)
    md = F(F(bt0 + msc[0, k - 1]) + tsc[k - 1, MD])
    d = F(F(bt0 + msc[0, first]) + tsc[first, MD])
    for j in range(first + 1, k - 1):
        tsc[j, DD] = F(-0.125)
        d = F(d + tsc[j, DD])
    tsc[k - 1, DD] = solve(lambda t: F(d + t), md, F(md - d))
    assert tsc[k - 1, DD] <= 0
    return TieCase("D: M before D", msc, isc, tsc, consts, codes, [(1, 2, k - 1, k + 1, b"MDM")],
                   [[(1, 2, first, k + 1, b"M" + b"D" * (chain + 1) + b"M")]])


# ---- E(i) = max_k M(i,k): the smallest k ----------------------------------------------------------------------------

def e_takes_the_smallest_k(leng, ks):
    """One residue, the same planted score at every node of `ks` (in any order): M(1,k) == E(1) on all of them."""
    msc, isc, tsc, consts, codes = _start(leng, 1, min(ks), 1, leng)
    assert max(ks) <= leng and len(set(ks)) == len(ks) >= 2
    for k in ks:
        msc[0, k] = F(2.0)
    lo = min(ks)
    return TieCase("E: smallest k", msc, isc, tsc, consts, codes, [(1, 1, lo, lo, b"M")],
                   [[(1, 1, k, k, b"M")] for k in sorted(ks) if k != lo])


# ---- the specials; the anchor is the node of the domains ------------------------------------------------------------

def _flag_differs(e1, e2, loop, candidates, want_from_e):
    """A constant t of `candidates` for which X(2) = max(fl(fl(e1 + t) + loop), fl(e2 + t)) takes E strictly
    (want_from_e) -- the OTHER special's flag on the tied row then differs from the tied one's (loop)."""
    for t in candidates:
        xl, xe = F(F(e1 + t) + loop), F(e2 + t)
        if (xe > xl) if want_from_e else (xl > xe):
            return F(t)
    raise AssertionError("no constant makes the two flags differ")


def c_takes_the_loop_before_e(leng, k):
    """a b: C(2) = max(C(1) + loop, E(2) + tEC) with the two equal: the domain at residue 1, not at residue 2.
    tr_E_J (still out of reach) is chosen so that J(2) takes E strictly: the row's J flag differs from its C flag."""
    msc, isc, tsc, consts, codes = _start(leng, 2, k, 1, leng)
    tBM, tEC = consts[0], consts[1]
    msc[0, k] = F(-2.0)                          # (the tied score is then coarser than the solved match score)
    loop, move = (F(x) for x in msv.sequence_transitions(2))
    e1 = F(entry(2, tBM, 0) + msc[0, k])
    cl = F(F(e1 + tEC) + loop)
    bt1 = entry(2, tBM, 1)
    msc[1, k] = solve(lambda e: F(F(bt1 + e) + tEC), cl, F(F(cl - tEC) - bt1))
    tEJ = _flag_differs(e1, F(bt1 + msc[1, k]), loop, [F(-50.0 - 0.1 * j) for j in range(200)], True)
    return TieCase("C: loop before E", msc, isc, tsc, (tBM, tEC, tEJ), codes, [(1, 1, k, k, b"M")],
                   [[(2, 2, k, k, b"M")]])


def j_takes_the_loop_before_e(leng, k):
    """a b c d, tr_E_J = -0.5: a domain at residue 1 feeds J, a last domain at residue 4 is entered from J.
    J(2) = max(J(1) + loop, E(2) + tEJ) with the two equal, E(2) itself entered from J(1): J loops over residue 2
    rather than passing through a domain there.  tr_E_C is chosen so that C(2) takes E strictly."""
    msc, isc, tsc, consts, codes = _start(leng, 4, k, 1, leng)
    tBM, tEJ = consts[0], F(-0.5)
    msc[3, k] = F(8.0)
    loop, move = (F(x) for x in msv.sequence_transitions(4))
    for first in (4.0, 4.125, 4.25, 4.375, 4.5):  # (a sum that falls half-way between floats skips every other one)
        msc[0, k] = F(first)
        e1 = F(entry(4, tBM, 0) + msc[0, k])
        j1 = F(e1 + tEJ)
        assert j1 > loop                         # B(1) comes from J
        bt1 = entry(4, tBM, 1, B=F(j1 + move))
        jl = F(j1 + loop)
        try:
            msc[1, k] = solve(lambda e: F(F(bt1 + e) + tEJ), jl, F(F(jl - tEJ) - bt1))
            break
        except AssertionError:
            continue
    else:
        raise AssertionError("no exact tie for any first domain")
    tEC = _flag_differs(e1, F(bt1 + msc[1, k]), loop, [F(-0.5 - 0.01 * j) for j in range(200)], True)
    return TieCase("J: loop before E", msc, isc, tsc, (tBM, tEC, tEJ), codes, [(1, 1, k, k, b"M"), (4, 4, k, k, b"M")],
                   [[(1, 1, k, k, b"M"), (2, 2, k, k, b"M"), (4, 4, k, k, b"M")]])


def b_takes_n_before_j(leng, k):
    """a b, tr_E_J = -0.75 != tr_E_C: B(1) = max(N(1) + move, J(1) + move) with the two equal, J(1) fed by a domain
    at residue 1 that only J can continue: one domain at residue 2, entered from N."""
    msc, isc, tsc, consts, codes = _start(leng, 2, k, 1, leng)
    tBM, tEC = consts[0], consts[1]
    msc[1, k] = F(6.0)
    loop, move = (F(x) for x in msv.sequence_transitions(2))
    bt0 = entry(2, tBM, 0)
    bn = F(F(loop) + move)
    for tEJ in (F(-0.75), F(-0.7), F(-0.8), F(-0.9), F(-1.1)):  # (half-way sums skip every other float)
        try:
            msc[0, k] = solve(lambda e: F(F(F(bt0 + e) + tEJ) + move), bn, F(F(F(loop) - tEJ) - bt0))
            break
        except AssertionError:
            continue
    else:
        raise AssertionError("no exact tie for any tr_E_J")
    return TieCase("B: N before J", msc, isc, tsc, (tBM, tEC, tEJ), codes, [(2, 2, k, k, b"M")],
                   [[(1, 1, k, k, b"M"), (2, 2, k, k, b"M")]])


class Rule(NamedTuple):
    build: object       # build(leng, k) -> TieCase
    first: int          # the first anchor the rule allows
    tail: int           # the last one is LENG - tail


# the eleven anchored rules (E, anchored at a set of nodes, is e_takes_the_smallest_k) and the variants with
# informative insert scores
RULES = {
    "M: M before I": Rule(m_takes_m_before_i, 2, 0),
    "M: M before D": Rule(m_takes_m_before_d, 3, 0),
    "M: M before B": Rule(m_takes_m_before_b, 2, 0),
    "M: I before D": Rule(m_takes_i_before_d, 3, 0),
    "M: I before D, insert scores": Rule(lambda leng, k: m_takes_i_before_d(leng, k, True), 3, 0),
    "M: I before B": Rule(m_takes_i_before_b, 2, 0),
    "M: D before B": Rule(m_takes_d_before_b, 3, 0),
    "I: M before I": Rule(i_takes_m_before_i, 1, 1),
    "I: M before I, insert scores": Rule(lambda leng, k: i_takes_m_before_i(leng, k, True), 1, 1),
    "D: M before D": Rule(d_takes_m_before_d, 3, 1),
    "C: loop before E": Rule(c_takes_the_loop_before_e, 1, 0),
    "J: loop before E": Rule(j_takes_the_loop_before_e, 1, 0),
    "B: N before J": Rule(b_takes_n_before_j, 1, 0),
}
ANCHORED_RULES = 11


def smallest_cases():
    """Every rule at the smallest LENG that holds it (the I and D rules at LENG = first + 1; E at LENG 2)."""
    out = [r.build(max(r.first + r.tail, 1), r.first) for r in RULES.values()]
    return out + [e_takes_the_smallest_k(2, (1, 2)), e_takes_the_smallest_k(3, (3, 1, 2))]


def anchored_cases(leng, anchors):
    """Every rule at each of `anchors` that it allows in a model of LENG `leng`, and at its first and last anchor."""
    for name, r in RULES.items():
        last = leng - r.tail
        for k in sorted({a for a in anchors if r.first <= a <= last} | {r.first, last}):
            yield name, k, r.build(leng, k)


def prove(case, best_path=None, dp_score=None):
    """The case's own proof, with neither trace under test: expected and every alternative are legal, different,
    and re-score to the same bits -- those of the explicit enumeration `best_path` (LENG <= 5) or of the DP score
    `dp_score`, a maximum that both paths then attain.  Returns the score."""
    leng, L = case.msc.shape[1] - 1, len(case.codes)
    assert L <= 6 and case.alternatives
    assert np.all(case.tsc[1:leng] <= 0)
    sc = rescore(*case.tables, case.codes, case.expected)
    check_legal(case.expected, leng, L)
    for alt in case.alternatives:
        check_legal(alt, leng, L)
        assert alt != case.expected
        assert bits(rescore(*case.tables, case.codes, alt)) == bits(sc), (case.rule, alt)
    if leng <= 5:
        assert bits(best_path(*case.tables, case.codes)) == bits(sc), case.rule
    else:
        assert bits(dp_score(*case.tables, case.codes)) == bits(sc), case.rule
    return sc
