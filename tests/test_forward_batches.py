"""CPU checks of tests/forward_batches.py: the models and batches that tests/test_gpu_forward_boundaries.py runs
really put their scores on the states, transitions and scan steps they are aimed at -- by far more than the GPU
tolerance (msv.h), so that an error there cannot hide under it -- and the ordinary batches do not.

Each check removes one thing from the model (a long D chain, a match column, one transition) and measures how far
the float64 score moves, in units of forward_lib.tolerance.  The thresholds are conditions on the constructions,
set before anything was measured; the figures seen are in the docstrings."""
import numpy as np
import pytest

from hmm_fasta_viterbi_amd.synthetic import concat_batches, gapped_homolog_batch, homolog_batch, random_batch
from forward_batches import (DD, MI, MM, aimed_batch, base_model, boundary_states, bridge_model, bridge_plan,
                             bridge_sequences, emissions, insertion_batch, knocked, with_transition)
from forward_lib import cpu_scores, np_forward, tolerance
from state_batches import knock_out, window_core

ALL_S = (2, 6, 12, 22, 38)


def split(codes, offsets):
    return [codes[int(offsets[i]):int(offsets[i + 1])] for i in range(len(offsets) - 1)]


def moved(model, other, codes, offsets):
    """Per sequence: |score - score on the other model| in units of the GPU tolerance, float64 library Forward."""
    full = cpu_scores(*model, codes, offsets)
    cut = cpu_scores(*other, codes, offsets)
    L = np.diff(offsets.astype(np.int64))
    with np.errstate(invalid="ignore"):
        d = np.abs(full - cut)
    d[np.isinf(full) & np.isinf(cut)] = 0.0
    return d / tolerance(L, model[0].shape[1] - 1, full)


# ---- the restated D chain ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("d_reach", [None, 0, 1, 6, 7, 8, 13, 40, 500])
def test_scanned_d_chain_equals_the_loops(d_reach):
    """np_forward's d_scan restatement (one accumulate, windowed for a cut) against its loops over states and over
    steps, at window widths below, at and above the block edges, and against the library's float64 Forward."""
    model = bridge_model(2, 5)
    codes, offsets = concat_batches(bridge_sequences(model, 2, 6), random_batch(7, 2, 1, 20))
    lib = cpu_scores(*model, codes, offsets)
    for q, s in enumerate(split(codes, offsets)):
        a = np_forward(*model, s, d_reach=d_reach)
        b = np_forward(*model, s, d_reach=d_reach, d_scan=True)
        assert abs(a - b) <= 1e-10 * max(1.0, abs(a)), (d_reach, q, a, b)
        if d_reach is None or d_reach >= 128:
            assert abs(lib[q] - b) <= 1e-9 * max(1.0, abs(b)), (d_reach, q, lib[q], b)


# ---- bridges -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("S", ALL_S)
def test_bridge_layout(S):
    """Sources alternate between a lane's first and last slot, every chain is longer than S (2^j + 1) d->d steps,
    everything lies at least 8 states inside the model, and every transition column is distinct per node."""
    plan = bridge_plan(S)
    assert [(s - 1) % S for s, _ in plan] == [0, S - 1] * 3
    assert {((s - 1) % S, (k - 1) % S) for s, k in plan} == {(0, 0), (S - 1, 0), (0, S - 1), (S - 1, S - 1)}
    for j, (s, k) in enumerate(plan):
        assert k - s - 2 > S * (2 ** j + 1) and (k - 1) // S - (s + 1 - 1) // S > 2 ** j
        assert s - 7 >= 1 and k + 7 <= 64 * S - 8
    msc, isc, tsc, consts = bridge_model(S, 3, inserts=True)
    assert msc.shape == (20, 64 * S + 1) and isc.shape == msc.shape and tsc.shape == (64 * S + 1, 7)
    for col in range(7):
        # (the six sources share m->d 0.5 and the six landings d->m 0.9; float32 draws may coincide)
        assert len(np.unique(tsc[1:64 * S, col])) >= 0.97 * (64 * S - 1) - 5, col
    dd = np.exp(tsc[1:64 * S, DD].astype(np.float64))  # nodes 1 .. LENG - 1
    toll = dd < 0.99
    assert 8 + 6 <= toll.sum() <= 26 + 12 and np.all((dd[toll] >= 0.7 - 1e-6) & (dd[toll] <= 0.9 + 1e-6))
    assert all(toll[((k - 2) // S - 1) * S:((k - 2) // S) * S].any() for _, k in plan)  # the lane left of a landing's
    assert all(toll[k - 2 - 1] for _, k in plan)  # (dd[i] is node i + 1) the d->d into each bridge's last D state
    assert dd[~toll].min() >= 0.999 - 1e-6 and dd.max() <= 0.9999 + 1e-6 and np.prod(dd[~toll][:1300]) > 0.45
    cross = np.diff(bridge_sequences((msc, isc, tsc, consts), S, 4, flank=0, cross=True)[1].astype(np.int64))
    assert len(cross) >= 17 and np.all(cross == 16)
    lens = np.diff(bridge_sequences((msc, isc, tsc, consts), S, 4)[1].astype(np.int64))
    assert len(lens) == 6 and lens.min() >= 16 and lens.max() <= 22


@pytest.mark.parametrize("S", ALL_S)
def test_bridge_sequences_depend_on_their_scan_step(S):
    """With every D chain cut after d_reach = S (2^j + 1) d->d steps -- all that the scan's steps below j deliver --
    the sequence of bridge j moves by at least 1,000 tolerances, every j.  Seen: 36,000-63,000 at S = 2,
    16,000-26,000 at S = 6, 7,600-14,000 at S = 12, 4,600-7,500 at S = 22, 2,000-4,200 at S = 38."""
    model = bridge_model(S, 11)
    leng = 64 * S
    codes, offsets = bridge_sequences(model, S, 12)
    lib = cpu_scores(*model, codes, offsets)
    seen = []
    for j, s in enumerate(split(codes, offsets)):
        assert len(s) <= 30
        full = np_forward(*model, s, d_scan=True)
        assert abs(full - lib[j]) <= 1e-9 * abs(full), (S, j, full, lib[j])
        cut = np_forward(*model, s, d_scan=True, d_reach=S * (2 ** j + 1))
        seen.append(abs(full - cut) / tolerance(len(s), leng, full))
        # the bridge's own chain carries that: it is back at the reach of exactly its k - s - 2 d->d steps and gone
        # one step below (what longer chains still add are the free D -> E exits downstream of the last match)
        sj, kj = bridge_plan(S)[j]
        at, below = (np_forward(*model, s, d_scan=True, d_reach=kj - sj - 2 - x) for x in (0, 1))
        assert (at - below) / tolerance(len(s), leng, full) >= 1000.0, (S, j, at, below)
    print(f"S = {S}: bridges moved by", [int(x) for x in seen], "tolerances")
    assert min(seen) >= 1000.0, (S, seen)


# ---- tails, heads, windows -----------------------------------------------------------------------------------------

def lengths(S):
    """The three lengths test_gpu_forward_boundaries.py runs, with the seed of its model at each."""
    return [(64 * S, 31), (64 * S - S + 1, 32), (64 * S - S, 33)]


@pytest.mark.parametrize("S", ALL_S)
@pytest.mark.parametrize("short", [0, 1, 2])
def test_tails_and_heads_depend_on_the_end_states(S, short):
    """LENG 64 S, 64 S - S + 1 and 64 S - S, the GPU test's models and batch: knocking out match column LENG moves
    at least half of the 24 tail homologs by at least 100 tolerances, and column 1 the head homologs.  Seen: tails
    16-23 of 24, heads 18-22 of 24 (the fewest at S = 22 and 38, where the tolerance is largest)."""
    leng, seed = lengths(S)[short]
    model = base_model(leng, seed)
    (codes, offsets), where = aimed_batch(model, S, 32)
    assert len(where["tail"]) == 24 and len(where["head"]) == 24
    for kind, state in (("tail", leng), ("head", 1)):
        ko = (knock_out(model[0], state),) + model[1:]
        w = moved(model, ko, codes, offsets)[where[kind]]
        print(f"S = {S}, LENG {leng}: {kind} homologs moved >= 100 tolerances by state {state}: "
              f"{int(np.sum(w >= 100.0))}/24")
        assert np.sum(w >= 100.0) >= 12, (S, leng, kind, w)


@pytest.mark.parametrize("S", ALL_S)
@pytest.mark.parametrize("short", [0, 1, 2])
def test_windows_depend_on_their_boundary(S, short):
    """LENG 64 S, 64 S - S + 1 and 64 S - S: with m->m of the boundary node b at -inf (the transition the next
    lane's first slot reads through MM_IN), every window across b | b + 1 moves by at least 1,000 tolerances, the
    ones the model's end clips included.  Seen: 19,000-73,000 at S = 2, 7,400-33,000 at S = 6, 3,700-18,000 at
    S = 12, 2,200-9,700 at S = 22, 1,200-6,000 at S = 38; the smallest of each is the window at LENG 64 S - S + 1
    that has state LENG alone beyond its boundary.  Before base_model gave states 1 and LENG one residue at 0.97
    that window moved by 846 tolerances at S = 38: a lone state earns its best match score and no more."""
    leng, seed = lengths(S)[short]
    model = base_model(leng, seed)
    (codes, offsets), where = aimed_batch(model, S, 32)
    bounds = boundary_states(leng, S)
    assert len(where["window"]) == len(bounds) >= 4
    seen = []
    assert np.diff(offsets.astype(np.int64))[where["edge"]].tolist() == [0, 1, 2, 63, 64, 65]
    for i, b in zip(where["window"], bounds):
        first, last = window_core(max(0, b - 12), 24, leng)
        assert first <= b < last <= leng
        s = codes[int(offsets[i]):int(offsets[i + 1])]
        w = moved(model, with_transition(model, MM, -np.inf, b), s, np.array([0, len(s)], np.uint64))[0]
        seen.append(int(w))
        assert w >= 1000.0, (S, leng, b, w)
    print(f"S = {S}, LENG {leng}: windows moved by", seen, "tolerances")


# ---- insertions ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("S", ALL_S)
@pytest.mark.parametrize("short", [0, 1, 2])
@pytest.mark.parametrize("inserts", [False, True])
def test_insertions_depend_on_their_node(S, short, inserts):
    """LENG 64 S, 64 S - S + 1 and 64 S - S, the GPU test's models and batch, with and without informative insert
    scores: with m->i of the insertion's node at -inf every insertion sequence moves by at least 100 tolerances.
    Measured when the builder was written: 490-44,000 tolerances at S = 2, 380-21,000 at S = 6, 380-16,000 at
    S = 12, 410-5,700 at S = 22, 220-4,700 at S = 38.  With uniform inserted residues and insertions of 3-4 residues
    beside a clipped side the smallest was 9, hence _insert_residues and the shorter insertions there; and at
    LENG 64 S - S + 1 the insertions after node LENG - 1, with state LENG alone beyond them, moved by 31-98 for
    S >= 12, hence _lone_state_pays, which leaves those out and keeps the ones at S = 2 and 6 and some at S = 12."""
    leng, seed = lengths(S)[short]
    model = base_model(leng, seed, inserts)
    (codes, offsets), nodes = insertion_batch(model, S, 42)
    slots = sorted(set((nodes - 1) % S))
    assert len(nodes) >= 16 and slots == ([0, 1] if S == 2 else [0, S - 1])  # first and last slots of a lane
    if short == 0:
        assert len(nodes) == 24
    worst, best = np.inf, 0.0
    for q, s in enumerate(split(codes, offsets)):
        w = moved(model, with_transition(model, MI, -np.inf, int(nodes[q])), s, np.array([0, len(s)], np.uint64))[0]
        worst, best = min(worst, w), max(best, w)
    print(f"S = {S}, LENG {leng}, inserts {inserts}: {len(nodes)} insertion sequences moved by {worst:.0f} .. "
          f"{best:.0f} tolerances")
    assert worst >= 100.0, (S, leng, inserts, worst)


# ---- the gap these batches close -----------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["write_hmm", "base_model"])
def test_ordinary_batches_do_not_reach_the_last_state(which, tmp_path):
    """On a 2,432-state model none of the uniform, homolog_batch and gapped_homolog_batch sequences of
    test_every_variant_at_exact_fit's batch (random starts) moves by more than 1 tolerance when column LENG is
    knocked out: on that test's own model (write_hmm, seed 900 + LENG) and on base_model."""
    leng = 2432
    if which == "write_hmm":
        import hmm_fasta_viterbi_amd as msv
        from hmm_fasta_viterbi_amd.synthetic import write_hmm
        from forward_lib import tables
        path = str(tmp_path / f"{leng}.hmm")
        write_hmm(path, leng, 900 + leng)
        h = msv.Profile_HMM(path)
        model, me = tables(h, 0), h.match_emissions
    else:
        model = base_model(leng, 51)
        me = emissions(model)
    codes, offsets = concat_batches(random_batch(40 + leng, 10, 1, 300), homolog_batch(me, 41 + leng, 10, 1, 300),
                                    gapped_homolog_batch(me, 42 + leng, 10, 1, 300))
    w = moved(model, (knock_out(model[0], leng),) + model[1:], codes, offsets)
    assert w.max() <= 1.0, w


# ---- knocked-out nodes ---------------------------------------------------------------------------------------------

def test_knocked_node_stops_every_path():
    """knocked(): a bridge whose chain crosses the node loses its path: its score falls by at least 1,000
    tolerances.  (The others move too: the free D -> E exits downstream of their last match stop at the node.)"""
    S = 6
    model = bridge_model(S, 61)
    codes, offsets = bridge_sequences(model, S, 62)
    node = 32 * S
    crosses = np.array([s < node < k for s, k in bridge_plan(S)])
    assert crosses.any() and not crosses.all()
    ko = knocked(model, node)
    assert np.all(np.isneginf(ko[0][:, node])) and np.all(np.isneginf(ko[2][node, [2, 5, 6]]))
    assert np.array_equal(model[2][node + 1], ko[2][node + 1]) and np.isfinite(model[2][node]).all()
    w = moved(model, ko, codes, offsets)
    assert np.all(w[crosses] >= 1000.0), w
    # the two float64 references agree on a model with zeros in it
    lib = cpu_scores(*ko, codes, offsets)
    for q, s in enumerate(split(codes, offsets)):
        want = np_forward(*ko, s)
        assert abs(lib[q] - want) <= 1e-9 * abs(want), (q, lib[q], want)
