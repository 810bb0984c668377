"""The batches of the split stage's GPU tests carry weight (split_lib; msv.h "Split stage"), shown on the
CPU twin alone and on THE SAME batches: every entry of split_lib.PLAN -- the models, junctions and seeds that
tests/test_gpu_split.py runs on all ten variants -- and the 100.hmm batch of its pipeline test.  The twin is the
float64 decode for the region rule and the region test, the float64 Forward with D rounded to float32 once under the
exponents the device's rule gives (split_lib.as_float32) for the sampler, and THE definitions msv_dom_regions,
msv_dom_is_multidomain, msv_spl_sample and msv_spl_cluster.  Nothing here was tuned on the GPU."""
import os

import numpy as np
import pytest

import hmm_fasta_viterbi_amd as msv
import decode_lib
import forward_lib
from split_lib import (DRAWS, PLAN, SEED, as_float32, copies_batch, cpu_ensemble, cpu_forward, device_exponents,
                       draws_on_rescaled_rows, gpu_batches, sample)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = sorted(PLAN)


def test_the_plan_covers_every_gpu_model_with_room_for_a_copy():
    want = {(S, ins, w) for S in (2, 6, 12, 22, 38) for ins in (False, True) for w in range(3)} - {(2, False, 2),
                                                                                                    (2, True, 2)}
    assert set(PLAN) == want


def _posteriors(model, codes, offsets, s):
    ref = decode_lib.cpu_decode_batch(*model, codes, offsets)
    off = offsets.astype(np.int64)
    return tuple(ref[k][off[s]:off[s + 1]].astype(np.float32) for k in (2, 3, 4))


def _two_copies(model, batch):
    (codes, offsets), planted, cores = batch
    off = offsets.astype(np.int64)
    b, e, o = _posteriors(model, codes, offsets, 0)
    regs = msv.dom_regions(b, e, o)
    assert len(regs) == 1, regs  # no linker: ONE region
    r = regs[0]
    assert r["i_from"] <= planted[0][0] + 2 and r["i_to"] >= planted[1][1] - 2
    assert msv.dom_is_multidomain(b, e, int(r["i_from"]), int(r["i_to"]))
    env_codes = codes[off[0] + int(r["i_from"]) - 1:off[0] + int(r["i_to"])]
    segs, per, _ = cpu_ensemble(model, env_codes, int(off[1] - off[0]), 0, int(r["i_from"]), 200, SEED)
    env = msv.spl_cluster(segs, 200)
    assert len(env) == 2, env
    for c, (first, last), other in zip(env, planted, cores[::-1]):
        inside = min(int(c["i_to"]), last) - max(int(c["i_from"]), first) + 1
        assert inside >= 0.8 * (last - first + 1), (c, first, last)
        assert int(c["i_to"]) < other[0] or int(c["i_from"]) > other[1], (c, other)  # no residue of the other core
    assert list(env["i_from"]) == sorted(env["i_from"])
    # the single-copy control is one region and not multi-domain
    b, e, o = _posteriors(model, codes, offsets, 1)
    regs = msv.dom_regions(b, e, o)
    assert len(regs) == 1
    assert not msv.dom_is_multidomain(b, e, int(regs[0]["i_from"]), int(regs[0]["i_to"]))


@pytest.mark.parametrize("key", KEYS)
def test_two_copies_are_one_region_that_splits_in_two(key):
    model, batch, _ = gpu_batches(*key)
    _two_copies(model, batch)


def test_the_pipeline_batch_of_100_hmm():
    model = forward_lib.tables(msv.Profile_HMM(os.path.join(ROOT, "data", "profile_HMMs", "100.hmm")))
    for seed in (910, 911):
        _two_copies(model, copies_batch(model, seed=seed))


@pytest.mark.parametrize("key", KEYS)
def test_every_special_draw_meets_a_rescale(key):
    """On the strong homolog some sample draws each of C <- E, J <- E, the J loop and M <- B on a row whose exponent
    differs from the row before; no row's E is within 2^0.02 of the rule's 2^32, sixteen times the largest device
    error the recorded values may have (16 (Le + LENG) 2^-24 <= 2.7e-3 relative here), so the device rescales on the
    same rows."""
    model, _, seq = gpu_batches(*key)
    st, _, *mat = cpu_forward(model, seq, len(seq))
    assert st == 0
    expo, margin = device_exponents(mat[3], mat[4])
    assert margin > 0.02 and expo[-1] >= 96  # several rescales
    planes = as_float32(*mat)
    samples = []
    for j in range(65):
        s, _, _, trunc = sample(model, planes, len(seq), 0, 1, len(seq), j, SEED)
        assert not trunc
        samples.append(s)
    met = draws_on_rescaled_rows(planes[3], samples)
    for k in DRAWS:
        assert met[k] >= 1, (k, met)
