"""The aimed inputs of the domain stage's GPU tests carry weight -- shown on the CPU, in units of the posterior
tolerance of msv.h (48 (L + LENG) 2^-24 + 8 2^-24, absolute).

The GPU comparison of begin / end / occ is held to a tolerance, so an error has to move a posterior by more than it to
be seen.  forward_batches.py's batches hang each sequence on one thing; here the float64 CPU decode runs with that
thing removed, and the posteriors move by at least 100 tolerances:
  * bridges: a node closed in the middle of the D chain (every bridge);
  * tails and heads: column LENG, column 1 closed (at least half of 24 each, the condition of
    test_forward_batches.py: a core is emitted with 10 % of its residues replaced and lies beside a uniform flank, so
    not every sequence's alignment reaches the end column with most of its mass);
  * windows across a lane boundary: the boundary node closed (knocked: match column, d->d, m->d, d->m), so that no
    path crosses it and the window falls into two domains -- every window;
  * insertions at a lane's edge: m->i closed at every node of the insertion's 24-state window, so that no I state
    can take the inserted residues and the sequence breaks into two domains or misaligns -- every insertion.
For the last two, closing ONE transition (m->m at the boundary, m->i of the one node) is not enough: the path goes
round through the neighbouring state, begin / end / occ -- probabilities on the special states -- hardly move (printed:
4-19 tolerances for the windows at S = 12), and only the Backward score shows it (printed too).  That is why the removal
asserted on is the one the sequence cannot go round.  A posterior is at most 1, so all this is shown where 100
tolerances are well below 1: S = 2, 6 and 12 (LENG <= 768).  At S = 38 the tolerance is 7e-3 and only a posterior that
flips can show it; the GPU tests run every variant all the same.

It also establishes the ROBUST SET of the region tests (decode_batches.robust): among the region batch's sequences
that have a region, at least three quarters keep every comparison the rule makes farther from its threshold than the
tolerance, in float64 -- on those the device regions must be the float64 regions."""
import numpy as np
import pytest

from decode_batches import REGION_SEED, REGION_SHAPES, region_batch, region_model, robust
from decode_lib import cpu_decode, np_regions, post_tolerance
from forward_lib import tolerance
from forward_batches import (MI, MM, aimed_batch, base_model, boundary_states, bridge_model, bridge_plan,
                             bridge_sequences, insertion_batch, knocked, with_transition)
from state_batches import knock_out

SHAPES = [(2, False), (6, False), (6, True), (12, False)]


def moved(model, altered, codes):
    """max over begin / end / occ and the residues of |posterior - posterior on the altered model|, in tolerances."""
    a, b = cpu_decode(*model, codes), cpu_decode(*altered, codes)
    assert a[0] == 0 and b[0] == 0
    tol = post_tolerance(len(codes), model[0].shape[1] - 1)
    with np.errstate(invalid="ignore"):
        return max(float(np.nanmax(np.abs(x - y))) for x, y in zip(a[3:], b[3:])) / tol


def score_moved(model, altered, codes):
    """|Backward score - Backward score on the altered model| in units of Forward's tolerance (msv.h), which the GPU
    tests hold the Backward score to."""
    a, b = cpu_decode(*model, codes), cpu_decode(*altered, codes)
    return abs(a[2] - b[2]) / float(tolerance(len(codes), model[0].shape[1] - 1, a[2]))


def split(codes, offsets):
    return [codes[int(offsets[i]):int(offsets[i + 1])] for i in range(len(offsets) - 1)]


@pytest.mark.parametrize("S,isc", SHAPES)
def test_bridges_hang_on_their_chain(S, isc):
    model = bridge_model(S, 11, isc)
    seqs = split(*bridge_sequences(model, S, 71, flank=1))
    w = [moved(model, knocked(model, (s + k) // 2), q) for (s, k), q in zip(bridge_plan(S), seqs)]
    print(f"S = {S}: a node closed mid-chain moves the bridges' posteriors by", np.round(w), "tolerances")
    assert min(w) >= 100.0


@pytest.mark.parametrize("S,isc", SHAPES)
def test_capacity_edges_hang_on_the_last_and_first_column(S, isc):
    for leng in (64 * S, 64 * S - S + 1, 64 * S - S):
        model = base_model(leng, 31, isc)
        (codes, offsets), where = aimed_batch(model, S, 32)
        seqs = split(codes, offsets)
        for kind, column in (("tail", leng), ("head", 1)):
            closed = (knock_out(model[0], column), *model[1:])
            w = np.array([moved(model, closed, seqs[i]) for i in where[kind]])
            print(f"S = {S}, LENG {leng}: column {column} closed moves {int((w >= 100).sum())} of {len(w)} {kind} "
                  f"homologs by >= 100 tolerances (median {np.median(w):.0f})")
            assert (w >= 100.0).sum() * 2 >= len(w)
        bounds = boundary_states(leng, S)
        # the boundary node closed: no path crosses the boundary, the window falls into two domains
        win = [seqs[i] for i in where["window"]]
        w = np.array([moved(model, knocked(model, b), q) for b, q in zip(bounds, win)])
        print(f"S = {S}, LENG {leng}: the boundary node closed moves the windows' posteriors by", np.round(w),
              "tolerances")
        assert w.min() >= 100.0
        # (for the record: m->m alone closed is gone round through I or D)
        cut = [with_transition(model, MM, -np.inf, node=b) for b in bounds]
        print(f"    m->m alone closed: posteriors by", np.round([moved(model, c, q) for c, q in zip(cut, win)]),
              "tolerances, Backward score by", np.round([score_moved(model, c, q) for c, q in zip(cut, win)]),
              "Forward tolerances")


def without_i_states(model, node, reach=12):
    """m->i closed at the nodes within `reach` of `node` (insertion_batch's window: 24 states around the boundary)."""
    leng = model[0].shape[1] - 1
    for k in range(max(1, node - reach), min(leng - 1, node + reach) + 1):
        model = with_transition(model, MI, -np.inf, node=k)
    return model


@pytest.mark.parametrize("S,isc", SHAPES)
def test_insertions_hang_on_the_i_states_of_their_window(S, isc):
    model = base_model(64 * S, 31, isc)
    (codes, offsets), nodes = insertion_batch(model, S, 42)
    seqs = split(codes, offsets)
    w = np.array([moved(model, without_i_states(model, int(k)), q) for k, q in zip(nodes, seqs)])
    print(f"S = {S}: no I state in the window moves the insertions' posteriors by {w.min():.0f} .. {w.max():.0f} "
          f"tolerances")
    assert w.min() >= 100.0
    # (for the record: m->i of the one node closed is gone round through the neighbouring node's I state)
    cut = [with_transition(model, MI, -np.inf, node=int(k)) for k in nodes]
    pw = np.array([moved(model, c, q) for c, q in zip(cut, seqs)])
    sw = np.array([score_moved(model, c, q) for c, q in zip(cut, seqs)])
    print(f"    m->i of the node alone closed: posteriors by {pw.min():.1f} .. {pw.max():.0f} tolerances "
          f"({int((pw >= 100).sum())} of {len(pw)} by >= 100), Backward score by {sw.min():.0f} .. {sw.max():.0f} "
          f"Forward tolerances")


@pytest.mark.parametrize("S,isc", REGION_SHAPES)
def test_three_quarters_of_the_region_sequences_are_robust(S, isc):
    model = region_model(S, isc)
    (codes, offsets), planted = region_batch(model, REGION_SEED + S)
    lens = np.diff(offsets.astype(np.int64))
    assert post_tolerance(lens.max(), 64 * S) <= 1.5e-3 and 64 * S <= 384
    ref, ok = robust(model, codes, offsets)
    off = offsets.astype(np.int64)
    found = np.array([len(np_regions(ref[2][off[s]:off[s + 1]], ref[3][off[s]:off[s + 1]], ref[4][off[s]:off[s + 1]]))
                      for s in range(len(off) - 1)])
    have = found > 0
    print(f"S = {S}{'i' if isc else ''}: {int(have.sum())} of {len(have)} sequences have a region, "
          f"{int((ok & have).sum())} of them robust; regions found per planted count: "
          f"{ {int(k): found[planted == k].tolist() for k in (1, 2)} }")
    assert have.sum() >= len(have) * 3 // 4  # the plants are found
    assert (ok & have).sum() * 4 >= have.sum() * 3
