"""The definition of the emit stage IS the model (msv.h "Emit stage"): on tiny profiles every outcome
(state path, residues) that msv_emit_generate emits has the frequency the model gives it -- a plain product of the
parsed probabilities, enumerated in Python (tests/emit_lib.py) -- within the binomial 5 sigma + 1 / N + K 2^-24, K the
draws on the outcome (the thresholds' quantisation), and no outcome of probability 0 occurs; any slice of any call is
reproducible; on the bundled profiles every truth replays; and the pooled statistics of 100.hmm's sample are the
model's.  Seeds are fixed: a failure is a bug, never chance."""
import numpy as np
import pytest

import hmm_fasta_viterbi_amd as msv
from emit_lib import DATA, Model, op_coordinates, outcomes_of, replay, tiny_profile

N = 28000
CUTOFF = 1e-4
CONFIGS = [(0, False, msv.INSERTS_ZERO), (0, True, msv.INSERTS_LOG_ODDS), (1, True, msv.INSERTS_ZERO),
           (2, False, msv.INSERTS_LOG_ODDS)]


def _check(profile, Lc, multihit, insert_mode, seed):
    model = Model(profile, Lc, multihit, insert_mode)
    batch = msv.emit_generate(profile, N, seed, length=Lc, multihit=multihit, insert_mode=insert_mode)
    assert not batch[5].any()
    counts = {}
    for o in outcomes_of(*batch[:5]):
        counts[o] = counts.get(o, 0) + 1
    expected = model.enumerate(CUTOFF)
    worst = 0.0
    for o in set(counts) | set(expected):
        p, draws = model.outcome_prob(o)
        assert p > 0.0, ("an outcome of probability 0 was emitted", o)
        if o not in expected:
            # below the enumeration's cutoff (N p < 3: the binomial bound is not a Gaussian's there); this also
            # shows the enumeration complete
            assert p < CUTOFF, (o, p)
            continue
        assert abs(expected[o] - p) <= 1e-12 * p, (o, expected[o], p)
        f = counts.get(o, 0) / N
        sigma = np.sqrt(p * (1.0 - p) / N)
        slack = 1.0 / N + draws * 2.0 ** -24
        assert abs(f - p) <= 5.0 * sigma + slack, (o, f, p)
        worst = max(worst, max(0.0, abs(f - p) - slack) / sigma)
    mass = sum(expected.values())
    return worst, len(expected), mass


@pytest.mark.parametrize("Lc", [0, 1, 2])
@pytest.mark.parametrize("multihit", [False, True])
def test_leng_1(tmp_path, Lc, multihit):
    worst, n, mass = _check(tiny_profile(tmp_path, 1), Lc, multihit, msv.INSERTS_ZERO, 11 + Lc)
    print(f"emit paths LENG 1 Lc {Lc} multihit {multihit}: {n} outcomes, mass {mass:.4f}, worst z = {worst:.2f}")


@pytest.mark.parametrize("config", CONFIGS)
@pytest.mark.parametrize("kind", ["plain", "closed", "loopy", "nodelete"])
@pytest.mark.parametrize("leng", [2, 3])
def test_tiny_models(tmp_path, leng, kind, config):
    Lc, multihit, insert_mode = config
    worst, n, mass = _check(tiny_profile(tmp_path, leng, kind), Lc, multihit, insert_mode, 97 * leng + Lc)
    print(f"emit paths LENG {leng} {kind} Lc {Lc} multihit {multihit} inserts {insert_mode}: {n} outcomes, "
          f"mass {mass:.4f}, worst z = {worst:.2f}")


def test_closed_transitions_never_fire(tmp_path):
    """`closed`: no I follows M(1); `nodelete`: no D follows M(1)."""
    for kind, banned in (("closed", "I"), ("nodelete", "D")):
        _, _, _, doms, ops, _ = msv.emit_generate(tiny_profile(tmp_path, 3, kind), N, 5, length=0)
        seen = 0
        for d in doms[doms["k_from"] == 1]:
            o = ops[int(d["ops_begin"]):int(d["ops_begin"]) + int(d["ops_len"])].tobytes().decode()
            assert len(o) < 2 or o[1] != banned, (kind, o)
            seen += len(o) >= 2
        assert seen > 1000
        print(f"emit paths {kind}: {seen} domains leave M(1), none through {banned}")


def _slices_equal(whole, part, at):
    codes, off, doff, doms, ops, trunc = whole
    pc, po, pdo, pd, pops, pt = part
    m = len(po) - 1
    c0, d0 = int(off[at]), int(doff[at])
    assert np.array_equal(pc, codes[c0:int(off[at + m])])
    assert np.array_equal(po, off[at:at + m + 1] - off[at])
    assert np.array_equal(pdo, doff[at:at + m + 1] - doff[at])
    assert np.array_equal(pt, trunc[at:at + m])
    w = doms[d0:int(doff[at + m])]
    for f in ("i_from", "i_to", "k_from", "k_to", "ops_len"):
        assert np.array_equal(pd[f], w[f])
    assert np.array_equal(pd["seq"] + at, w["seq"])
    o0 = int(w["ops_begin"][0]) if len(w) else 0
    assert np.array_equal(pd["ops_begin"] + o0, w["ops_begin"])
    assert np.array_equal(pops, ops[o0:o0 + len(pops)])


@pytest.mark.parametrize("first", [0, (1 << 32) + 12345])
def test_slices_reproduce(first):
    profile = msv.Profile_HMM(f"{DATA}/100.hmm")
    whole = msv.emit_generate(profile, 300, 42, first, length=50)
    for at, m in ((0, 1), (7, 64), (299, 1), (100, 200)):
        _slices_equal(whole, msv.emit_generate(profile, m, 42, first + at, length=50), at)
    base = whole[0][:int(whole[1][50])].tobytes()
    for other in (dict(seed=43), dict(length=51), dict(multihit=False), dict(insert_mode=msv.INSERTS_LOG_ODDS)):
        kw = dict(seed=42, length=50)
        kw.update(other)
        seed = kw.pop("seed")
        got = msv.emit_generate(profile, 50, seed, first, **kw)
        assert got[0].tobytes() != base, other


def _structure(batch, leng, unihit, max_length=None):
    codes, off, doff, doms, ops, trunc = batch
    n = len(off) - 1
    L = np.diff(off).astype(np.int64)
    if max_length is None:
        assert not trunc.any()
    else:
        assert np.array_equal(trunc, L == max_length) and L.max() <= max_length
    assert codes.max() < 20
    assert np.all(doms["k_from"] >= 1) and np.all(doms["k_to"] <= leng) and np.all(doms["k_from"] <= doms["k_to"])
    assert np.all(doms["i_from"] >= 1) and np.all(doms["i_from"] <= doms["i_to"])
    assert np.array_equal(doms["seq"], np.repeat(np.arange(n), np.diff(doff).astype(np.int64)))
    assert np.all(doms["i_to"] <= L[doms["seq"]])
    # replaying the ops from (i_from, k_from) ends at (i_to, k_to); every k on the way is in 1 .. LENG
    dom, i, k = op_coordinates(doms, ops)
    last = doms["ops_begin"].astype(np.int64) + doms["ops_len"].astype(np.int64) - 1
    assert np.array_equal(i[last], doms["i_to"]) and np.array_equal(k[last], doms["k_to"])
    assert k.min() >= 1 and k.max() <= leng
    assert np.array_equal(doms["ops_begin"][1:], (doms["ops_begin"] + doms["ops_len"])[:-1])
    assert doms["ops_begin"][0] == 0
    assert int(doms["ops_begin"][-1] + doms["ops_len"][-1]) == len(ops)
    assert np.all(ops[doms["ops_begin"].astype(np.int64)] == ord("M"))
    # domains disjoint and in order within a sequence
    same = doms["seq"][1:] == doms["seq"][:-1]
    assert np.all(doms["i_from"][1:][same] > doms["i_to"][:-1][same])
    # the last op is M or D and no I sits at k_to -- but for a domain that max_length cut
    cut = np.zeros(len(doms), bool)
    if max_length is not None:
        cut = trunc[doms["seq"]] & (doms["i_to"] == L[doms["seq"]])
    assert np.all(ops[last][~cut] != ord("I"))
    at_exit = (ops == ord("I")) & (k == doms["k_to"][dom]) & ~cut[dom]
    assert not at_exit.any()
    if unihit:
        nd = np.diff(doff)
        assert np.all(nd[~trunc] == 1) and np.all(nd <= 1)
    inside = np.zeros(n, np.int64)
    np.add.at(inside, doms["seq"], doms["i_to"].astype(np.int64) - doms["i_from"].astype(np.int64) + 1)
    assert np.all(inside <= L)
    return L - inside


@pytest.mark.parametrize("name,n", [("100", 3000), ("1400", 400), ("2405", 300)])
def test_structure_on_bundled_profiles(name, n):
    profile = msv.Profile_HMM(f"{DATA}/{name}.hmm")
    leng = profile.model_length - 1
    for multihit in (True, False):
        for insert_mode in (msv.INSERTS_ZERO, msv.INSERTS_LOG_ODDS):
            batch = msv.emit_generate(profile, n, 42, multihit=multihit, insert_mode=insert_mode)
            outside = _structure(batch, leng, not multihit)
            print(f"emit structure {name}.hmm multihit {multihit} inserts {insert_mode}: {len(batch[3])} domains, "
                  f"{len(batch[4])} ops, mean length {np.diff(batch[1]).mean():.1f}, outside {outside.mean():.1f}")
    # truncation: 1, 2 and a length that falls inside a domain (Lc = 0: the first residue opens one)
    for cut in (1, 2, 17):
        batch = msv.emit_generate(profile, 200, 9, length=0, max_length=cut)
        _structure(batch, leng, False, cut)
        L = np.diff(batch[1])
        assert batch[5].any() and np.all(L[batch[5]] == cut)
        if cut == 17:
            d = batch[3][np.flatnonzero(batch[5])[0] == batch[3]["seq"]][-1]
            assert replay(d, batch[4]) == (int(d["i_to"]), int(d["k_to"]))
    batch = msv.emit_generate(profile, 200, 9, length=400, max_length=1)
    assert np.all(np.diff(batch[1]) == 1) and batch[5].all()
    _structure(batch, leng, False, 1) if len(batch[3]) else None


def test_pooled_statistics_on_100():
    """The residues M(k) emits against row k and the fragment ends, each within the binomial 5 sigma (+ 1 / n and the
    quantisation) per cell, and the mean flank length against Lc / 3 within 5 sigma of a geometric law's mean.  N is
    chosen so that the definition passes; the seed is fixed."""
    profile = msv.Profile_HMM(f"{DATA}/100.hmm")
    leng, Lc, n = profile.model_length - 1, 100, 20000
    codes, off, doff, doms, ops, trunc = msv.emit_generate(profile, n, 2024, length=Lc)
    assert not trunc.any()
    model = Model(profile, Lc, True, msv.INSERTS_ZERO)
    dom, i, k = op_coordinates(doms, ops)
    is_m = ops == ord("M")
    res = codes[off[doms["seq"]].astype(np.int64)[dom[is_m]] + i[is_m] - 1]
    table = np.zeros((leng + 1, 20), np.int64)
    np.add.at(table, (k[is_m], res), 1)
    visits = table.sum(axis=1)
    worst = 0.0
    for kk in range(1, leng + 1):
        p = model.mat[kk]
        sigma = np.sqrt(p * (1 - p) / visits[kk])
        dev = np.abs(table[kk] / visits[kk] - p)
        slack = 1.0 / visits[kk] + 2.0 ** -24
        assert np.all(dev <= 5 * sigma + slack), (kk, visits[kk])
        worst = max(worst, float(np.max(np.maximum(dev - slack, 0) / np.maximum(sigma, 1e-300))))
    print(f"emit pooled: {int(visits.sum())} match residues, worst emission z = {worst:.2f}")
    nd = len(doms)
    ks = np.arange(1, leng + 1)
    ends = (("k_from", np.bincount(doms["k_from"], minlength=leng + 1)[1:], (leng - ks + 1) / model.npairs),
            ("k_to", np.bincount(doms["k_to"], minlength=leng + 1)[1:], ks / model.npairs))
    for name, got, p in ends:
        sigma = np.sqrt(p * (1 - p) / nd)
        dev = np.abs(got / nd - p)
        slack = 1.0 / nd + 2.0 ** -24
        assert np.all(dev <= 5 * sigma + slack), name
        print(f"emit pooled: {nd} domains, worst {name} z = {float(np.max(np.maximum(dev - slack, 0) / sigma)):.2f}")
    inside = np.zeros(n, np.int64)
    np.add.at(inside, doms["seq"], doms["i_to"].astype(np.int64) - doms["i_from"].astype(np.int64) + 1)
    flanks = nd + n
    mean = float((np.diff(off).astype(np.int64) - inside).sum()) / flanks
    sigma = np.sqrt(model.loop) / model.move / np.sqrt(flanks)
    print(f"emit pooled: {flanks} flanks, mean length {mean:.3f} against {Lc / 3:.3f}, sigma {sigma:.3f}")
    assert abs(mean - Lc / 3.0) <= 5 * sigma + 2.0 ** -24 * Lc
    assert abs(nd / n - 2.0) <= 5 * np.sqrt(2.0 / n)  # a geometric number of domains: mean 2, variance 2
