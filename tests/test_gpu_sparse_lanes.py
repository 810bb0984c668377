"""Decode, align, null2 and split on the GPU where most lanes hold no state.

The four stages run one item per 64-lane wave, lane l holding states l S + 1 .. l S + S, and their own suites force
every variant onto models that nearly fill it.  Here every variant meets the models of sparse_lane_batches.py -- the
first model the automatic choice gives it (64 S' + 1; LENG 3 at S = 2), LENG 32 S + 1 (node LENG alone in lane 32, the
one source lane of the scans' 32-lane step) and LENG 17 S (node LENG in the last slot of lane 16) -- and the bundled
profiles that sit in the same place meet their automatic variants.  One profile per model, the four stages on the same
batch, each held to the checks ITS OWN module defines (imported, not copied) with msv.h's bounds as functions of
(L or Le, LENG): no tolerance is new here, and every bit-for-bit comparison stays bit for bit.  On top of those:
no domain and no sampled segment leaves nodes 1 .. LENG; the same items under the next larger variant, where the
model ends in lane 0 - 20, stay within the same bounds and give the same regions on the sequences whose
rule comparisons are robust in float64; a workspace of exactly the largest item gives the one-chunk bytes.  The worst
shares of the bounds are printed by the imported checks before they are asserted; DESIGN 4.10 - 4.14 record them."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import hmm_fasta_viterbi_amd as msv
from hmm_fasta_viterbi_amd import _native
from hmm_fasta_viterbi_amd.synthetic import concat_batches, gapped_homolog_batch, homolog_batch, random_batch

import decode_lib
import forward_lib
import test_gpu_align
import test_gpu_decode
import test_gpu_null2
import test_gpu_split
from decode_batches import robust
from decode_lib import np_regions
from forward_batches import base_model
from null2_lib import R
from oracle_lib import bits
from sparse_lane_batches import (KINDS, case, lanes_used, larger, null2_case, null2_refs, sparse_lengths,
                                 with_spoiled)
from state_batches import _csr
from test_gpu_decode import VARIANTS, shape_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = test_gpu_split.NS


class Stages(test_gpu_decode.Profile, test_gpu_align.Profile, test_gpu_null2.Profile, test_gpu_split.Profile):
    """ONE raw domain profile over a model's tables with the four modules' calls on it (decode, align, run, sample).
    `name` is forced, or with forced=False expected of the automatic choice.  On entry the three describe calls are
    checked as the four helpers check them: the variant, its S, and that no kernel of any stage spills."""

    def __init__(self, model, name, forced=True):
        self.model, self.name, self.forced = model, name, forced

    def __enter__(self):
        S, isc = shape_of(self.name)
        assert (self.model[1] is not None) == isc
        self.p = decode_lib.create_profile(*self.model, self.name if self.forced else None)
        try:
            self.info = decode_lib.describe(self.p)
            assert self.info["variant"] == self.name and self.info["states_per_lane"] == S, self.info
            assert self.info["scratch_bytes"] == 0 and self.info["model_length"] == self.model[0].shape[1], self.info
            aln, spl = _native.AlnInfo(), _native.SplInfo()
            assert _native.lib().msv_aln_describe(self.p, C.byref(aln)) == 0
            assert _native.lib().msv_spl_describe(self.p, C.byref(spl)) == 0
            aln, spl = aln.as_dict(), spl.as_dict()
            assert aln["variant"] == self.name.replace("dom_", "aln_") and aln["states_per_lane"] == S, aln
            assert spl["variant"] == self.name.replace("dom_", "spl_") and spl["states_per_lane"] == S, spl
            assert aln["null2_row_block"] == R
            for k in ("forward", "backward", "fill", "walk", "null2_partial", "null2_finish"):
                assert aln[k + "_scratch_bytes"] == 0, aln
            assert spl["forward_scratch_bytes"] == 0 and spl["sample_scratch_bytes"] == 0, spl
        except BaseException:
            decode_lib.destroy_profile(self.p)
            raise
        return self

    def __exit__(self, *exc):
        decode_lib.destroy_profile(self.p)


def forward_variant_of(model):
    """What a raw msv_fwd_profile over the model, created with no variant name, says it is."""
    f = forward_lib.create_profile(*model)
    try:
        info = _native.FwdInfo()
        assert _native.lib().msv_fwd_profile_describe(f, info) == 0
        return info.variant.decode()
    finally:
        forward_lib.destroy_profile(f)


def domain_variant_of(model):
    p = decode_lib.create_profile(*model)
    try:
        return decode_lib.describe(p)["variant"]
    finally:
        decode_lib.destroy_profile(p)


def run_stages(p, batch, null2_batch, what):
    """The four stages on one profile, each under its own module's checks; then what only makes sense here: nothing
    outside the model.  Returns the results by stage."""
    model = p.model
    leng = model[0].shape[1] - 1
    codes, offsets, items = batch
    # decode: scores, posteriors, regions; the recording kernel's score has the Forward kernel's bits
    env, ref, _ = test_gpu_decode.check_against_cpu(p, codes, offsets, f"decode {what}")
    f = forward_lib.create_profile(*model, p.name.replace("dom_", "fwd_"))
    try:
        st, want = forward_lib.gpu_scores(f, codes, offsets)
        assert st == 0
    finally:
        forward_lib.destroy_profile(f)
    st, got = decode_lib.gpu_scores(p.p, codes, offsets)
    assert st == 0 and np.array_equal(bits(got), bits(want)), what
    assert np.array_equal(bits(env.forward_scores), bits(want)), what
    # align
    aln = test_gpu_align.check_items(p, codes, offsets, items, f"align {what}", forward_bits=True)
    # null2 (its own stretches: the row blocks' edges), one item with a bad residue
    _, c2, o2, i2, bad, refs = null2_batch
    n2 = test_gpu_null2.check_null2(p, model, c2, o2, i2, bad, refs, f"null2 {what}")
    # split: the recorded matrix, the samples; its envelope scores are the alignment stage's
    spl = test_gpu_split.check_items(p, codes, offsets, items, f"split {what}", strong=None)
    assert np.array_equal(bits(spl["env"]), bits(aln["env"])), what
    # nothing outside the model: every domain and every sampled segment within nodes 1 .. LENG.  The planes the
    # alignment stage hands over have LENG + 1 columns: padding slots are never copied out, column 0 is the host's zero
    for out in (aln, n2):
        d = out["domains"]
        assert len(d) and d["k_from"].min() >= 1 and d["k_to"].max() <= leng and np.all(d["k_from"] <= d["k_to"]), what
        for (s, a, b), post in zip(items if out is aln else i2, out["post"]):
            assert post[0].shape == post[1].shape == (b - a + 1, leng + 1), what
            assert not post[0][:, 0].any() and not post[1][:, 0].any(), what
    g = spl["segments"]
    assert len(g) and g["k_from"].min() >= 1 and g["k_to"].max() <= leng and np.all(g["k_from"] <= g["k_to"]), what
    return {"env": env, "aln": aln, "null2": n2, "spl": spl}


def check_one_chunk_bytes(p, batch, null2_batch, results, what):
    """A workspace of exactly the largest item: several chunks, the one-chunk bytes, for decode, align + null2 and
    split."""
    S, _ = shape_of(p.name)
    codes, offsets, items = batch
    L = _native.lib()
    longest = int(np.diff(offsets.astype(np.int64)).max())
    cut = p.decode(codes, offsets, workspace_bytes=int(L.msv_dom_sequence_bytes(longest)))
    assert cut.stats["chunks"] > 1 and results["env"].stats["chunks"] == 1
    test_gpu_decode.assert_same_bits(cut, results["env"])
    _, c2, o2, i2, bad, _ = null2_batch
    one = p.run(c2, o2, i2, status=4)
    cut = p.run(c2, o2, i2, status=4, workspace_bytes=max(int(L.msv_aln_item_bytes(S, b - a + 1)) for _, a, b in i2))
    assert cut["stats"]["chunks"] > 1 and one["stats"]["chunks"] == 1
    for f in test_gpu_null2.FIELDS + ("null2", "domcorr"):
        assert cut[f].tobytes() == one[f].tobytes() == results["null2"][f].tobytes(), (what, f)
    one = p.sample(codes, offsets, items)
    cut = p.sample(codes, offsets, items,
                   workspace_bytes=max(int(L.msv_spl_item_bytes(S, b - a + 1)) for _, a, b in items))
    assert cut["stats"]["chunks"] > 1 and one["stats"]["chunks"] == 1 and cut["stats"]["truncated"] == 0
    for f in ("env", "sample_off", "segments"):
        assert cut[f].tobytes() == one[f].tobytes() == results["spl"][f].tobytes(), (what, f)


@pytest.mark.parametrize("name", VARIANTS)
def test_sparse_lanes(name):
    """The three sparse models of the variant's S; each again under the next larger variant of the same insert mode
    (S = 38 has none), and the one-chunk bytes on the `lane 32 alone` model."""
    S, isc = shape_of(name)
    wider = None if larger(S) is None else VARIANTS[VARIANTS.index(name) + 1]
    assert wider is None or shape_of(wider) == (larger(S), isc)
    for which, kind in enumerate(KINDS):
        model, codes, offsets, items, where = case(S, isc, which)
        batch, null2_batch = (codes, offsets, items), null2_case(S, isc, which)
        leng = model[0].shape[1] - 1
        assert leng == sparse_lengths(S)[which]
        what = f"{name} LENG {leng} ({kind}, {lanes_used(leng, S)} lanes)"
        if which == 0:
            # the first model the automatic choice gives this variant, on both raw profile types; one node fewer
            # is the previous variant's last
            assert domain_variant_of(model) == name and forward_variant_of(model) == name.replace("dom_", "fwd_")
            if S > 2:
                below = base_model(leng - 1, 70, isc)
                smaller = VARIANTS[VARIANTS.index(name) - 1]
                assert domain_variant_of(below) == smaller
                assert forward_variant_of(below) == smaller.replace("dom_", "fwd_")
        with Stages(model, name) as p:
            mine = run_stages(p, batch, null2_batch, what)
            if which == 1:
                check_one_chunk_bytes(p, batch, null2_batch, mine, what)
        if wider is None:
            continue
        # independence of the padding: the same items under the next larger variant, the same bounds; the regions
        # of the sequences that are robust in float64 are the float64 regions under both
        with Stages(model, wider) as p:
            theirs = run_stages(p, batch, null2_batch,
                                f"{wider} LENG {leng} ({kind}, {lanes_used(leng, larger(S))} lanes)")
        ref, ok = robust(model, codes, offsets)
        off = offsets.astype(np.int64)
        compared = 0
        for s in np.flatnonzero(ok):
            a, b = (tuple((int(r["i_from"]), int(r["i_to"])) for r in x["env"].regions_of(s)) for x in (mine, theirs))
            assert a == b, (what, s, a, b)
            assert list(a) == np_regions(ref[2][off[s]:off[s + 1]], ref[3][off[s]:off[s + 1]],
                                         ref[4][off[s]:off[s + 1]]), (what, s)
            compared += len(a)
        print(f"{what}: {int(ok.sum())} robust sequences of {len(ok)}, {compared} regions equal under {wider}")
        assert ok.sum() >= len(ok) // 2 and compared >= 3, what


# ---- bundled profiles through their automatic variants -----------------------------------------------------------

BUNDLED = {"200.hmm": "dom_s6", "400.hmm": "dom_s12", "800.hmm": "dom_s22g", "1509.hmm": "dom_s38g4"}


def bundled_batch(hmm):
    """6 homologs and 2 gapped homologs of 60 - 130 residues on the profile's own match emissions, one concatenation
    of two of them, 3 uniform sequences; every sequence a whole item."""
    me = hmm.match_emissions
    hom, gap = homolog_batch(me, 21, 6, 60, 130), gapped_homolog_batch(me, 22, 2, 60, 130)
    two = _csr([hom[0][int(hom[1][0]):int(hom[1][2])]])
    codes, offsets = concat_batches(hom, gap, two, random_batch(23, 3, 60, 130))
    L = np.diff(offsets.astype(np.int64))
    return codes, offsets, [(s, 1, int(L[s])) for s in range(len(L))]


@pytest.mark.parametrize("mode", [msv.INSERTS_ZERO, msv.INSERTS_LOG_ODDS])
@pytest.mark.parametrize("prof", list(BUNDLED))
def test_bundled_profiles_through_their_automatic_variants(prof, mode):
    """200.hmm, 400.hmm, 800.hmm and 1509.hmm use 34, 34, 37 and 40 lanes of dom_s6, dom_s12, dom_s22g and dom_s38g4:
    the four stage checks through a raw profile over the PARSED tables (their -inf entries included), no variant
    forced; then the cascade with every domain stage on, against align_batch by hand."""
    hmm = msv.Profile_HMM(os.path.join(ROOT, "data", "profile_HMMs", prof))
    model = forward_lib.tables(hmm, mode)
    leng = hmm.model_length - 1
    name = BUNDLED[prof] + ("i" if mode else "")
    S, _ = shape_of(name)
    codes, offsets, items = bundled_batch(hmm)
    c2, o2, i2, bad = with_spoiled(model, codes, offsets, items)
    null2_batch = (model, c2, o2, i2, bad, null2_refs(model, c2, o2, i2, bad))
    with Stages(model, name, forced=False) as p:
        run_stages(p, (codes, offsets, items), null2_batch, f"{prof} on {name} ({lanes_used(leng, S)} lanes)")
    if mode != msv.INSERTS_ZERO:
        return
    engines = (msv.MSV_HMM(hmm, device=0), msv.Viterbi_HMM(hmm, device=0), msv.Forward_HMM(hmm, device=0))
    dom = msv.Domain_HMM(hmm, device=0)
    assert dom.describe()["variant"] == name
    out = msv.search_pipeline(*engines, codes=codes, offsets=offsets, dom_engine=dom, align=True, null2=True,
                              split=True)
    aln = out["alignments"]
    # (the bundled profiles are as weak per node as real ones: in float64 two to four of these short homologs have a
    # Forward P-value under the cascade's 1e-5, so the hits are few; test_sparse_lanes carries the strong ones)
    print(f"{prof}: {len(out['envelopes'])} hits, {len(aln)} alignment items")
    assert len(aln) >= 1 and aln.status == "MSV_OK" and out["split"]["ensembles"].stats["truncated"] == 0
    hand = dom.align_batch(codes=codes, offsets=offsets, items=aln.items, null2=True)
    for f in ("envelope_scores", "null2", "domcorrection"):
        assert getattr(hand, f).tobytes() == getattr(aln, f).tobytes(), (prof, f)
    assert aln.domains["k_from"].min() >= 1 and aln.domains["k_to"].max() <= leng
    dom.close()
