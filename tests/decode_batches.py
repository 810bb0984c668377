"""Models and batches for the domain stage's region tests (test helper; not a conftest), on top of forward_batches.py.

region_model / region_batch: sequences with one or two planted domains -- consensus runs of a model window with a few
mutations between uniform flanks -- whose envelopes the rule has to find.  The rule compares posteriors with thresholds,
and the device posteriors differ from the float64 ones within msv.h's tolerance, so a comparison closer to its
threshold than the tolerance may fall either way: robust() marks the sequences on which, in float64, every comparison
the rule makes lies farther from its threshold than the posterior tolerance.  tests/test_decode_batches.py asserts on
the CPU that three quarters of the sequences that have a region are robust; the GPU test compares regions on those.
The models stay small (LENG 128 and 384, L <= 130: tolerance <= 1.5e-3): at LENG 2,432 the tolerance is 1.3e-2 and
fewer than half of such sequences clear it."""
from __future__ import annotations

import numpy as np

from decode_lib import RT1, RT2, cpu_decode_batch, post_tolerance, rule_margin
from forward_batches import base_model, consensus
from state_batches import _csr

REGION_SHAPES = ((2, False), (2, True), (6, False), (6, True))  # (S, insert odds): dom_s2, dom_s2i, dom_s6, dom_s6i
# The batch of shape S is region_batch(model, REGION_SEED + S).  Over five seeds the float64 reference finds 22-30 of
# 32 sequences robust at S = 6 (28-32 at S = 2); this one leaves 28 at both S = 6 shapes, four above the three
# quarters the tests need, so another libm's last bits do not decide it.
REGION_SEED = 720


def region_model(S: int, inserts: bool):
    """forward_batches.base_model at LENG 64 S."""
    return base_model(64 * S, 500 + S, inserts)


def region_batch(model, seed: int, n_one: int = 16, n_two: int = 16, lmax: int = 130):
    """n_one sequences with one planted domain and n_two with two: a domain is the consensus of a window of 18..30
    states from a random start with 10 % of its residues replaced by uniform ones; flanks and the gap between two
    domains are 6..20 uniform residues; the whole at most lmax.  Returns ((codes, offsets), planted domain count)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    leng = model[0].shape[1] - 1

    def domain():
        core = int(rng.integers(18, 31))
        core = min(core, leng)
        start = int(rng.integers(1, leng - core + 2))
        d = consensus(model, start, start + core - 1).copy()
        flip = rng.random(core) < 0.10
        d[flip] = rng.integers(0, 20, size=int(flip.sum()), dtype=np.uint8)
        return d

    def flank():
        return rng.integers(0, 20, size=int(rng.integers(6, 21)), dtype=np.uint8)

    seqs, planted = [], []
    for k in [1] * n_one + [2] * n_two:
        parts = [flank()]
        for _ in range(k):
            parts += [domain(), flank()]
        s = np.concatenate(parts)
        assert len(s) <= lmax
        seqs.append(s)
        planted.append(k)
    return _csr(seqs), np.array(planted)


def robust(model, codes, offsets, rt1=RT1, rt2=RT2):
    """(the float64 reference of cpu_decode_batch, robust [n] bool): robust where every comparison the rule makes on
    the float64 posteriors lies farther from its threshold than msv.h's posterior tolerance."""
    ref = cpu_decode_batch(*model, codes, offsets)
    leng = model[0].shape[1] - 1
    off = offsets.astype(np.int64) - int(offsets[0])
    out = np.zeros(len(off) - 1, bool)
    for s in range(len(off) - 1):
        lo, hi = off[s], off[s + 1]
        out[s] = rule_margin(ref[2][lo:hi], ref[3][lo:hi], ref[4][lo:hi], rt1, rt2) > post_tolerance(hi - lo, leng)
    return ref, out
