"""The aimed batches of the alignment stage's GPU tests carry weight (conditions on the inputs, shown on the CPU twin
msv_aln_cpu_align): the optimal-accuracy paths of the bridge sequences hold D runs across the boundaries
of lanes 1, 16, 32 and 63, closing the crossed d->d gate changes the path, the insertion batch's paths hold I ops in a
lane's last slot, and the capacity-edge batch has a domain that ends in the model's last node and one that starts in
node 1 -- at every S of the variant family."""
import numpy as np
import pytest

from align_lib import cpu_align, path_key
from forward_batches import (BOUNDARY_LANES, DD, DM, MD, aimed_batch, base_model, bridge_model, bridge_plan,
                             bridge_sequences, consensus, insertion_batch)

SLOTS = (2, 6, 12, 22, 38)


def key_of(model, codes):
    st, score, oa, doms, ops, pp = cpu_align(model, codes)
    assert st == 0 and np.isfinite(oa)
    return path_key(doms, ops)


def d_runs(key):
    """[(first node, last node)] of every maximal run of D states of a path."""
    runs = []
    for dom in key:
        run = []
        for st, k, i in dom + (("M", 0, 0),):
            if st == "D":
                run.append(k)
            elif run:
                runs.append((run[0], run[-1]))
                run = []
    return runs


def boundary_bridge(model, S, lane):
    """A copy of `model` with one more bridge, across the boundary b | b + 1 of `lane` (b = lane S): m->d opened at
    node b - 1, d->m at the landing's left neighbour, as bridge_model opens its own; and the sequence that takes it:
    the consensus up to the source, then from the landing on (both clipped to the model)."""
    msc, isc, tsc, consts = model
    leng = msc.shape[1] - 1
    b = lane * S
    s, k = b - 1, min(b + 3, leng)
    tsc = tsc.copy()
    tsc[s, MD] = np.float32(np.log(0.5))
    tsc[k - 1, DM] = np.float32(np.log(0.9))
    codes = np.concatenate([consensus(model, max(1, s - 7), s), consensus(model, k, min(leng, k + 7))])
    return (msc, isc, tsc, consts), codes, b


@pytest.mark.parametrize("S", SLOTS)
def test_bridges_cross_the_lane_boundaries(S):
    model = bridge_model(S, 11, S in (6, 22))
    # the six planned bridges: one D run each from the source to the landing, the last across more than 32 lanes
    codes, offsets = bridge_sequences(model, S, 70, flank=1)
    for (s, k), lo, hi in zip(bridge_plan(S), offsets[:-1], offsets[1:]):
        runs = d_runs(key_of(model, codes[int(lo):int(hi)]))
        assert (s + 1, k - 1) in runs, (S, s, k, runs)
    assert max(k - s for s, k in bridge_plan(S)) > 32 * S
    for lane in BOUNDARY_LANES:
        bridged, seq, b = boundary_bridge(model, S, lane)
        key = key_of(bridged, seq)
        crossing = [r for r in d_runs(key) if r[0] <= b < r[1]]
        assert crossing, (S, lane, key)
        # the d->d out of node b is the step across the boundary: without it the path must differ
        msc, isc, tsc, consts = bridged
        closed = tsc.copy()
        closed[b, DD] = -np.inf
        other = key_of((msc, isc, closed, consts), seq)
        assert other != key and not [r for r in d_runs(other) if r[0] <= b < r[1]], (S, lane)


@pytest.mark.parametrize("inserts", (False, True))
@pytest.mark.parametrize("S", SLOTS)
def test_insertions_sit_in_a_lanes_last_slot(S, inserts):
    model = base_model(64 * S, 31, inserts)
    (codes, offsets), nodes = insertion_batch(model, S, 42)
    seen = set()
    for q, node in enumerate(nodes):
        if node % S:
            continue  # (the next lane's first slot)
        key = key_of(model, codes[int(offsets[q]):int(offsets[q + 1])])
        if any(st == "I" and k == node for dom in key for st, k, i in dom):
            seen.add(int(node) // S)
    assert len(seen) >= 2, (S, seen)  # I ops in the last slot of at least two of the three aimed lanes


@pytest.mark.parametrize("S", SLOTS)
def test_capacity_edge_domains_touch_both_ends(S):
    leng = 64 * S
    model = base_model(leng, 31, False)
    (codes, offsets), where = aimed_batch(model, S, 32)
    ends = starts = 0
    for q in np.concatenate([where["tail"][::4], where["head"][::4]]):
        st, score, oa, doms, ops, pp = cpu_align(model, codes[int(offsets[q]):int(offsets[q + 1])])
        assert st == 0
        ends += int(np.any(doms["k_to"] == leng))
        starts += int(np.any(doms["k_from"] == 1))
    assert ends >= 1 and starts >= 1, (S, ends, starts)
