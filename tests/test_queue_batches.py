"""queue_batches.py (the batches of test_gpu_queue_depth.py) on the CPU: the batch has exactly the size asked
for -- the tests' pigeonhole argument rests on it -- and the edge cases really sit deep in the queue, next to
the neighbours that make them matter (a short sequence after a long one on the same stream)."""
import time

import numpy as np
import pytest

import hmm_fasta_viterbi_amd as msv
from oracle_lib import profile_path
from queue_batches import (EDGE_LENGTHS, msv_capacity, msv_groups, msv_streams, prefix, queue_batch, take_sequences,
                           viterbi_capacity)

_me = {}


def match_emissions(prof="400.hmm"):
    if prof not in _me:
        _me[prof] = msv.Profile_HMM(profile_path(prof)).match_emissions
    return _me[prof]


@pytest.mark.parametrize("n", [20_000, 400_000])
def test_queue_batch_shape(n):
    t0 = time.perf_counter()
    codes, offsets = queue_batch(match_emissions(), 5, n)
    dt = time.perf_counter() - t0
    print(f"queue_batch n={n}: {dt:.2f} s, {codes.size} residues")
    assert codes.dtype == np.uint8 and offsets.dtype == np.uint64
    assert len(offsets) - 1 == n  # exact: n > capacity is the whole argument
    assert int(offsets[0]) == 0 and int(offsets[-1]) == codes.size
    assert codes.size == 0 or int(codes.max()) < 20
    lens = np.diff(offsets.astype(np.int64))
    assert lens.min() == 0 and lens.max() <= 130
    for e in EDGE_LENGTHS:  # every edge length deep in the queue, not only in the first round of the grid
        at = np.nonzero(lens == e)[0]
        assert len(at) >= 40 and at.max() >= n / 3, (e, at[-3:])
    odd = (lens & 1) == 1
    assert np.any(odd[:-1] & ~odd[1:]) and np.any(~odd[:-1] & odd[1:])  # two-row loops: both parities in a row
    after_long = np.concatenate([[False], lens[:-1] >= 64])
    assert np.any(after_long & (lens == 1)) and np.any(after_long & (lens == 0))
    c2, o2 = queue_batch(match_emissions(), 5, n)
    assert np.array_equal(codes, c2) and np.array_equal(offsets, o2)  # deterministic in the seed
    c3, o3 = queue_batch(match_emissions(), 6, n)
    assert not np.array_equal(offsets, o3)


def test_queue_batch_smallest_and_lmax():
    codes, offsets = queue_batch(match_emissions("100.hmm"), 1, 4000, lmax=70)
    lens = np.diff(offsets.astype(np.int64))
    assert len(lens) == 4000
    assert set(EDGE_LENGTHS) <= set(lens.tolist())  # the edge lengths do not depend on lmax
    with pytest.raises(ValueError):
        queue_batch(match_emissions("100.hmm"), 1, 300)


def test_take_sequences_and_prefix():
    codes, offsets = queue_batch(match_emissions("100.hmm"), 2, 3000)
    idx = np.array([7, 7, 0, 2999, 13], np.int64)
    c, o = take_sequences(codes, offsets, idx)
    assert len(o) == len(idx) + 1 and int(o[-1]) == c.size
    for k, i in enumerate(idx):
        assert np.array_equal(c[int(o[k]):int(o[k + 1])], codes[int(offsets[i]):int(offsets[i + 1])])
    c, o = take_sequences(codes, offsets, np.zeros(0, np.int64))
    assert c.size == 0 and np.array_equal(o, np.zeros(1, np.uint64))
    c, o = prefix(codes, offsets, 17)
    assert len(o) == 18 and c.size == int(offsets[17]) and np.array_equal(c, codes[:c.size])


def test_capacities():
    vit = {"blocks": 256, "waves_per_block": 12, "waves_per_sequence": 2}
    assert viterbi_capacity(vit) == 1536
    assert viterbi_capacity({**vit, "waves_per_block": 8, "waves_per_sequence": 1, "blocks": 1024}) == 8192
    info = {"blocks": 512, "waves_per_block": 8, "lanes_per_group": 16}
    assert msv_streams("msv_g16_s88_w8_p2_d2") == 2 and msv_streams("msv_g64_s34_a32_w16_p2_d1") == 1
    assert msv_groups(info) == 512 * 8 * 4
    assert msv_capacity(info, "msv_g16_s88_w8_p2_d2") == 2 * 512 * 8 * 4
    assert msv_capacity({**info, "lanes_per_group": 64}, "msv_g64_s4_w16_p1_d1") == 512 * 8
    with pytest.raises(ValueError):
        msv_streams("msv_g16_s8_w4_p2")
