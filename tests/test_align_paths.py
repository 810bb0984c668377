"""The alignment stage's CPU functions (msv.h "Alignment stage") against an explicit enumeration of every
state path of tiny models: LENG 1-4, Le 0-4, with and without insert odds.  The enumerator (align_lib) records each
residue's label, so the posteriors are plain sums over paths and the optimal-accuracy score is a plain maximum."""
import numpy as np
import pytest

from align_lib import (cpu_align, cpu_decode, enumerate_paths, enumerated_posteriors, labels_of, oa, path_accuracy,
                       path_key)
from forward_batches import base_model
from forward_lib import DD, DM, MD, MM

LENGS = (1, 2, 3, 4)
ENVELOPES = (0, 1, 2, 3, 4)


def _codes(leng, Le, seed):
    return np.random.Generator(np.random.PCG64(seed)).integers(0, 20, size=Le, dtype=np.uint8)


def _check(model, codes, Lc=None):
    Le, M = len(codes), model[0].shape[1]
    st, score, pm, pi, pn, pj, pc = cpu_decode(model, codes, Lc)
    assert st == 0
    if Le == 0:
        assert score == -np.inf
        got = oa(model, (pm, pi, pn, pj, pc), Lc)
        assert got[0] == -np.inf and len(got[1]) == 0 and len(got[2]) == 0
        return
    paths = enumerate_paths(model, codes, Lc)
    Z, *want = enumerated_posteriors(paths, Le, M)
    assert abs(score - np.log(Z)) <= 1e-10 * max(1.0, abs(np.log(Z)))
    for name, g, w in zip(("ppM", "ppI", "ppN", "ppJ", "ppC"), (pm, pi, pn, pj, pc), want):
        assert np.max(np.abs(g - w), initial=0.0) <= 1e-10, name
    rows = pm.sum(axis=1) + pi.sum(axis=1) + pn + pj + pc
    assert np.max(np.abs(rows - 1.0)) <= 1e-10

    # the definition, on the float64 posteriors rounded once: its score is the maximum over the enumerated paths
    post32 = tuple(np.asarray(x, np.float32) for x in (pm, pi, pn, pj, pc))
    post = tuple(x.astype(np.float64) for x in post32)
    score_oa, doms, ops, op_pp = oa(model, post32, Lc)
    acc = {key: path_accuracy(key, post) for key in paths}
    best = max(acc.values())
    tol = 4.0 * Le * 2.0 ** -24 * max(1.0, best)  # Le float32 adds of partial sums <= Le
    assert abs(float(score_oa) - best) <= tol, (score_oa, best)
    key = path_key(doms, ops)
    assert key in paths, key
    assert abs(acc[key] - best) <= tol
    # a domain starts and ends in M, and the reported posteriors are the cells' own
    total = 0.0
    at = 0
    for dom in key:
        assert dom[0][0] == "M" and dom[-1][0] == "M"
        for state, k, i in dom:
            want_pp = post32[0][i - 1, k] if state == "M" else post32[1][i - 1, k] if state == "I" else np.float32(0)
            assert op_pp[at] == want_pp
            total += float(op_pp[at])
            at += 1
    for i, lab in enumerate(labels_of(key, Le)):
        if isinstance(lab, str):
            total += float({"N": post32[2], "J": post32[3], "C": post32[4]}[lab][i])
    assert abs(total - float(score_oa)) <= tol
    # the twin is the decode rounded to float32 and then the definition: the same bits
    st, sc2, oa2, d2, o2, p2 = cpu_align(model, codes, Lc)
    assert st == 0 and sc2 == score and oa2 == score_oa
    assert path_key(d2, o2) == key and np.array_equal(p2, op_pp)


@pytest.mark.parametrize("inserts", (False, True))
@pytest.mark.parametrize("leng", LENGS)
def test_every_path_of_tiny_models(leng, inserts):
    model = base_model(leng, 4100 + leng, inserts)
    for Le in ENVELOPES:
        for rep in range(2):
            codes = _codes(leng, Le, 97 * leng + 11 * Le + rep)
            _check(model, codes)
            if Le:
                _check(model, codes, Lc=Le + 7)


@pytest.mark.parametrize("leng", (2, 4))
def test_consensus_envelopes(leng):
    """Residues the model likes: the mass sits on the core states, not on N and C."""
    model = base_model(leng, 4200 + leng, True)
    cons = np.argmax(model[0][:, 1:], axis=0).astype(np.uint8)
    for Le in (leng, min(4, leng + 1)):
        codes = np.resize(cons, Le)
        _check(model, codes)
        st, _, pm, pi, pn, pj, pc = cpu_decode(model, codes)
        assert pm.sum() > 0.5 * Le


def test_without_the_j_loop():
    """tr_E_J = -inf: no path has two domains, and the definition never reports two."""
    msc, isc, tsc, consts = base_model(3, 4300, True)
    model = (msc, isc, tsc, (consts[0], consts[1], -np.inf))
    for Le in (1, 2, 3, 4):
        codes = _codes(3, Le, 500 + Le)
        _check(model, codes)
        assert all(len(key) == 1 for key in enumerate_paths(model, codes))
        assert len(cpu_align(model, codes)[3]) == 1


def test_with_a_closed_node():
    """Every transition into node 3 closed: no path enters it except from B, which the definition must respect even
    where node 3's posteriors are the row's largest."""
    msc, isc, tsc, consts = base_model(4, 4400, False)
    tsc = tsc.copy()
    tsc[2, [MM, MD, DM, DD]] = -np.inf
    tsc[2, 3] = -np.inf  # i->m of node 2
    model = (msc, isc, tsc, consts)
    cons = np.argmax(msc[:, 1:], axis=0).astype(np.uint8)
    for codes in (cons, cons[:3], cons[1:], _codes(4, 4, 77)):
        _check(model, codes)
        for key in enumerate_paths(model, codes):
            for dom in key:
                for a, b in zip(dom, dom[1:]):
                    assert not (a[1] == 2 and b[1] == 3)
