"""The batches of tests/test_gpu_sparse_lanes.py carry weight (conditions on the inputs, shown on the float64 twins
alone; sparse_lane_batches.py): on every model whose last real lane is lane 16, 21-37 or 32 (lane 1 at LENG 3) some
item's optimal-accuracy path matches state LENG, some item's path matches both states of the last real lane's boundary,
some item's Forward score is far beyond the first rescale, and the two-copy sequence has a sample with two segments.
Nothing here was tuned on the GPU."""
import numpy as np
import pytest

from align_lib import cpu_align, path_key
from forward_batches import boundary_states
from sparse_lane_batches import KINDS, SLOTS, case, lanes_used, larger, null2_case, sparse_lengths
from split_lib import SEED, cpu_ensemble

NS = 65  # test_gpu_split.NS


def test_lengths_and_lanes():
    assert [sparse_lengths(S) for S in SLOTS] == [(3, 65, 34), (129, 193, 102), (385, 385, 204), (769, 705, 374),
                                                  (1409, 1217, 646)]
    for S in SLOTS:
        first, alone, ends = sparse_lengths(S)
        assert lanes_used(alone, S) == 33 and (alone - 1) % S == 0  # node LENG in lane 32's first slot
        assert lanes_used(ends, S) == 17 and ends % S == 0  # node LENG in lane 16's last slot
        assert max(first, alone, ends) <= 64 * S
        if S > 2:
            assert first - 1 == 64 * SLOTS[SLOTS.index(S) - 1] and 22 <= lanes_used(first, S) <= 38
        if larger(S):
            # under the next larger variant every model ends in the left third of the wave
            assert max(lanes_used(x, larger(S)) for x in (first, alone, ends)) <= 21
    assert [lanes_used(sparse_lengths(S)[0], S) for S in SLOTS] == [2, 22, 33, 35, 38]


@pytest.mark.parametrize("which", range(3), ids=[k.replace(" ", "_") for k in KINDS])
@pytest.mark.parametrize("inserts", (False, True))
@pytest.mark.parametrize("S", SLOTS)
def test_batches_reach_the_end_the_last_boundary_a_rescale_and_two_segments(S, inserts, which):
    model, codes, offsets, items, where = case(S, inserts, which)
    leng = model[0].shape[1] - 1
    assert leng == sparse_lengths(S)[which]
    off = offsets.astype(np.int64)
    b = (lanes_used(leng, S) - 1) * S  # boundary b | b + 1 on the left of the last real lane
    assert b in boundary_states(leng, S) and 1 <= b < leng
    ends = crossings = 0
    best = -np.inf
    for s, a, e in items:
        st, score, oa, doms, ops, pp = cpu_align(model, codes[off[s] + a - 1:off[s] + e], int(off[s + 1] - off[s]))
        assert st == 0
        matched = {k for dom in path_key(doms, ops) for op, k, i in dom if op == "M"}
        ends += leng in matched
        crossings += b in matched and b + 1 in matched
        best = max(best, score)
    two = where["two"]
    segs, per, _ = cpu_ensemble(model, codes[off[two]:off[two + 1]], int(off[two + 1] - off[two]), two, 1, NS, SEED)
    double = sum(len(s) == 2 for s, _, _ in per)
    print(f"S = {S}{'i' if inserts else ''} LENG {leng} ({lanes_used(leng, S)} lanes): {len(items)} items, {ends} "
          f"match state LENG, {crossings} match states {b} and {b + 1}, best Forward score {best:.1f} nats, "
          f"{double} of {NS} samples of the two-copy sequence have two segments")
    assert (22 if leng >= 24 else 15) <= len(items) <= 34  # about 25: the GPU cases stay quick
    assert ends >= 1 and crossings >= 1
    assert best > 5 * 22.2
    assert double >= 1


@pytest.mark.parametrize("S", SLOTS)
def test_null2_items_differ_only_in_their_stretches(S):
    model, codes, offsets, items, where = case(S, False, 1)
    m2, c2, o2, i2, bad, refs = null2_case(S, False, 1)
    assert bad == len(i2) - 1 and refs[bad] is None and all(r is not None for r in refs[:bad])
    shared = where["control"] + 1
    assert np.array_equal(offsets[:shared + 1], o2[:shared + 1]) and i2[:shared] == items[:shared]
    assert np.array_equal(codes[:int(offsets[shared])], c2[:int(o2[shared])])
    assert c2[int(o2[-2]):].max() == 21 and c2[:int(o2[-2])].max() < 20
