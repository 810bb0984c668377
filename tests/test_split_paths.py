"""The split stage's sampler (msv.h "Split stage") against an explicit enumeration of every state path of
tiny models: LENG 1-3, envelopes of 1-4 residues, with and without insert odds, one model with a closed node and one
with the J loop closed.  The float64 twin's matrix (msv_spl_cpu_forward), rounded to float32 with exponent 0, goes to
THE definition msv_spl_sample N times with the fixed seed; a path of probability p = odds / Z must be seen with
frequency within 5 sqrt(p (1 - p) / N) + 1 / N of p -- five standard deviations of the binomial count plus one count
for the float32 rounding of the matrix and the weights, whose relative effect on any p is below 1e-5 -- no sample may
fall outside the enumerated paths and none may be truncated.

N = 28,000: 5 sqrt(p / N) + 1 / N < p for every p >= 1e-3, so a path at least that likely cannot be missed altogether;
the bound is asserted on those paths, rarer ones are left to the "no impossible path" check.  The worst z (the
deviation over the binomial standard deviation) is printed."""
import numpy as np
import pytest

from align_lib import enumerate_paths
from forward_batches import base_model
from forward_lib import DD, DM, MD, MM
from split_lib import as_float32, cpu_forward, sample_counts

N = 28000
P_MIN = 1e-3


def _codes(Le, seed):
    return np.random.Generator(np.random.PCG64(seed)).integers(0, 20, size=Le, dtype=np.uint8)


def _check(model, codes, Lc=None, i_from=1, seq=0):
    Le = len(codes)
    Lc = Le + i_from - 1 if Lc is None else Lc
    st, score, *mat = cpu_forward(model, codes, Lc)
    assert st == 0
    assert np.all(mat[4] == 0)  # no rescale on these models: exponent 0
    paths = enumerate_paths(model, codes, Lc)
    Z = sum(paths.values())
    assert abs(score - np.log(Z)) <= 1e-10 * max(1.0, abs(np.log(Z)))
    got, truncated = sample_counts(model, as_float32(*mat), Lc, seq, i_from, i_from + Le - 1, N)
    assert truncated == 0
    assert sum(got.values()) == N
    worst = 0.0
    for key in got:
        assert key in paths, key
    for key, w in paths.items():
        p = w / Z
        if p < P_MIN:
            continue
        f = got.get(key, 0) / N
        sigma = np.sqrt(p * (1.0 - p) / N)
        if sigma > 0:
            worst = max(worst, abs(f - p) / sigma)
        assert abs(f - p) <= 5.0 * sigma + 1.0 / N, (key, f, p)
    return worst, len(paths)


@pytest.mark.parametrize("inserts", (False, True))
@pytest.mark.parametrize("leng", (1, 2, 3))
def test_every_path_of_tiny_models(leng, inserts):
    model = base_model(leng, 4100 + leng, inserts)
    worst = 0.0
    for Le in (1, 2, 3, 4):
        z, n_paths = _check(model, _codes(Le, 97 * leng + 11 * Le))
        worst = max(worst, z)
    print(f"split paths LENG {leng} inserts {inserts}: N = {N}, worst z = {worst:.2f}")


def test_an_envelope_inside_its_parent():
    """i_from > 1 and Lc > Le: the key and the loop odds are the parent's."""
    model = base_model(3, 4103, True)
    z, _ = _check(model, _codes(4, 311), Lc=11, i_from=5, seq=3)
    print(f"split paths inside a parent: N = {N}, worst z = {z:.2f}")


def test_without_the_j_loop():
    """tr_E_J = -inf: no path has two domains, and no sample has two."""
    msc, isc, tsc, consts = base_model(3, 4300, True)
    model = (msc, isc, tsc, (consts[0], consts[1], -np.inf))
    worst = 0.0
    for Le in (1, 2, 3, 4):
        codes = _codes(Le, 500 + Le)
        assert all(len(key) == 1 for key in enumerate_paths(model, codes))
        worst = max(worst, _check(model, codes)[0])
    print(f"split paths without J: N = {N}, worst z = {worst:.2f}")


def test_with_a_closed_node():
    """Every transition into node 3 closed: no sample enters it except from B."""
    msc, isc, tsc, consts = base_model(3, 4400, False)
    tsc = tsc.copy()
    tsc[2, [MM, MD, DM, DD]] = -np.inf
    tsc[2, 3] = -np.inf  # i->m of node 2
    model = (msc, isc, tsc, consts)
    cons = np.argmax(msc[:, 1:], axis=0).astype(np.uint8)
    worst = 0.0
    for codes in (cons, _codes(4, 77)):
        for key in enumerate_paths(model, codes):
            for dom in key:
                for a, b in zip(dom, dom[1:]):
                    assert not (a[1] == 2 and b[1] == 3)
        worst = max(worst, _check(model, codes)[0])
    print(f"split paths with a closed node: N = {N}, worst z = {worst:.2f}")
