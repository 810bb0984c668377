"""CPU checks of tests/state_batches.py: the batches the capacity-edge tests (test_gpu_state_boundaries.py)
rely on really depend on the states they are aimed at -- and the ordinary homolog batches do not.

Sensitivity is measured by knocking a state out: its emission column set to -inf with every constant kept (a
model written with LENG - 1 nodes would not do: tr_B_Mk depends on LENG, so every score would change), scored
by the CPU DPs over caller tables (numpy_msv, oracle_lib.vit_score_tables), which first have to equal the
oracle bitwise on the intact table."""
import numpy as np
import pytest

from hmm_fasta_viterbi_amd.synthetic import homolog_batch, random_batch, write_hmm
from oracle_lib import OracleProfile, bits, vit_score_tables
from state_batches import (boundary_batch, knock_out, numpy_msv, tail_gapped_batch, tail_homolog_batch,
                           window_core, window_homolog_batch)

LENGS = (96, 1408, 2432)
_models = {}


def model(leng, tmp_path_factory):
    """(oracle profile, MSV table, constants, Viterbi transitions) of the synthetic model (seed 7), made once."""
    if leng not in _models:
        path = str(tmp_path_factory.mktemp("state_batches") / f"syn{leng}.hmm")
        write_hmm(path, leng, 7)
        o = OracleProfile(path)
        _models[leng] = (o, o.emission_scores(), o.constants(), o.vit_tables(0)[1])
    return _models[leng]


def both_stages(leng, tmp_path_factory, codes, offsets, state):
    """Scores changed by knocking `state` out: (MSV, Viterbi) counts; the table DPs are first checked against
    the oracle on the intact tables."""
    o, es, consts, tsc = model(leng, tmp_path_factory)
    msv_intact = numpy_msv(es, *consts, codes, offsets)
    vit_intact = vit_score_tables(es, None, tsc, consts, codes, offsets)
    assert np.array_equal(bits(msv_intact), bits(o.score_batch(codes, offsets))), leng
    assert np.array_equal(bits(vit_intact), bits(o.vit_score_batch(codes, offsets))), leng
    ko = knock_out(es, state)
    return (bits(numpy_msv(ko, *consts, codes, offsets)) != bits(msv_intact),
            bits(vit_score_tables(ko, None, tsc, consts, codes, offsets)) != bits(vit_intact))


@pytest.mark.parametrize("leng", LENGS)
def test_tail_batches_depend_on_the_last_state(leng, tmp_path_factory):
    """At least half of 24 tail homologs change score when state LENG is knocked out, MSV and Viterbi; at least
    half of 24 gapped tail sequences change their Viterbi score when the last 13 states are."""
    o = model(leng, tmp_path_factory)[0]
    me = o.arrays()[0]
    codes, offsets = tail_homolog_batch(me, 11, 24, 8, 130)
    assert len(offsets) == 25 and int(np.diff(offsets).min()) >= 8 and int(np.diff(offsets).max()) <= 130
    m, v = both_stages(leng, tmp_path_factory, codes, offsets, leng)
    print(f"LENG {leng}: tail homologs changed by state LENG: MSV {int(m.sum())}/24, Viterbi {int(v.sum())}/24")
    assert m.sum() >= 12 and v.sum() >= 12, (leng, int(m.sum()), int(v.sum()))
    gc, go = tail_gapped_batch(me, 13, 24, 8, 130)
    # (half of these paths skip node LENG itself -- a D chain runs into it -- so the last 13 nodes are knocked out)
    _, gv = both_stages(leng, tmp_path_factory, gc, go, list(range(max(1, leng - 12), leng + 1)))
    print(f"LENG {leng}: gapped tail sequences changed by the last 13 states: Viterbi {int(gv.sum())}/24")
    assert gv.sum() >= 12, (leng, int(gv.sum()))


@pytest.mark.parametrize("leng", LENGS)
def test_window_batches_depend_on_their_core(leng, tmp_path_factory):
    """Every window homolog changes score when the middle state of its core is knocked out, MSV and Viterbi;
    windows that overhang the model's two ends are clipped to it."""
    me = model(leng, tmp_path_factory)[0].arrays()[0]
    starts = [0, leng // 3, leng // 2 - 12, leng - 30, leng - 24, leng - 5, -7]
    codes, offsets = window_homolog_batch(me, 17, starts, 24)
    assert len(offsets) - 1 == len(starts)
    for i, start in enumerate(starts):
        first, last = window_core(start, 24, leng)
        assert 1 <= first <= last <= leng and last - first + 1 <= 24
        assert last - first + 1 <= int(offsets[i + 1] - offsets[i]) <= last - first + 1 + 12
        if last - first + 1 < 24:
            continue  # clipped at an end of the model: too short to carry the path
        m, v = both_stages(leng, tmp_path_factory, codes[int(offsets[i]):int(offsets[i + 1])],
                           np.array([0, offsets[i + 1] - offsets[i]], np.uint64), (first + last) // 2)
        assert m[0] and v[0], (leng, start, first, last)


@pytest.mark.parametrize("leng", LENGS[1:])
def test_ordinary_homologs_do_not_reach_the_last_state(leng, tmp_path_factory):
    """The gap these batches close: none of 24 homolog_batch sequences (the seed of test_every_variant_matches_
    oracle) and none of 24 uniform ones changes score at 1408 / 2432 states when the last state is knocked out."""
    me = model(leng, tmp_path_factory)[0].arrays()[0]
    for codes, offsets in (homolog_batch(me, 22, 24, 8, 130), random_batch(7, 24, 8, 130)):
        m, v = both_stages(leng, tmp_path_factory, codes, offsets, leng)
        assert m.sum() == 0 and v.sum() == 0, (leng, int(m.sum()), int(v.sum()))


def test_boundary_batch_holds_every_kind():
    """boundary_batch: 24 tail homologs, one window per boundary inside the model, 12 gapped ones for Viterbi,
    the six edge lengths, 24 uniform sequences in between; the index map points at them."""
    rng = np.random.default_rng(3)
    me = np.vstack([np.zeros((1, 20)), rng.uniform(0.01, 1.0, (200, 20))])
    (codes, offsets), where = boundary_batch(me, 5, [0, 16, 100, 199, 200, 512], viterbi=True)
    lens = np.diff(offsets.astype(np.int64))
    assert len(where["tail"]) == 24 and len(where["window"]) == 3 and len(where["gapped"]) == 12
    assert lens[where["edge"]].tolist() == [0, 1, 2, 63, 64, 65]
    assert len(lens) == 24 + 3 + 12 + 6 + 24 and int(offsets[-1]) == codes.size and lens.max() <= 130
    assert codes.size and int(codes.max()) < 20
    # aimed sequences alternate with uniform ones
    aimed = np.concatenate([where["window"], where["tail"]])
    assert np.array_equal(aimed[:24], 2 * np.arange(24))  # the uniform ones sit at the odd indices between them
    (c2, o2), w2 = boundary_batch(me, 5, [0, 16, 100, 199, 200, 512], viterbi=False)
    assert "gapped" not in w2 and len(o2) - 1 == 24 + 3 + 6 + 24
