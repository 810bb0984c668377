"""The bias stage on the GPU (aln_null2.hip), every variant: the null2 model of each envelope by
expectation and its correction, against the library's float64 twin (msv_aln_cpu_null2) on the same tables.

Bounds are msv.h's ("Bias stage"): |null2_gpu[x] - null2_cpu[x]| <= delta_x = (48 (Le + LENG) + 2 (Le + 2 LENG + 8))
2^-24 null2_cpu[x] + W_x 2^-60, and the domcorrection within the bound that follows through the log (its input
condition is asserted for every item by tests/test_null2_host.py).  The device's domcorrection has no tolerance: it
equals msv_aln_null2_correction on the device's own null2 bit for bit; bias_scores equals msv_aln_bias_scores exactly;
results do not depend on the chunking, on an item's place or on the run.  The worst errors are printed before they are
asserted; DESIGN 4.12 records them."""
import ctypes as C
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import hmm_fasta_viterbi_amd as msv
from hmm_fasta_viterbi_amd import _native
from hmm_fasta_viterbi_amd.synthetic import concat_batches, homolog_batch, random_batch

import align_lib
import decode_lib
import null2_lib
from align_lib import post_bound
from forward_batches import base_model, queue_batch
from forward_lib import U
from null2_lib import R, case, correction, domcorr_bound, gpu_align_opts, null2_bound, odds32
from oracle_lib import bits
from state_batches import _csr

VARIANTS = ["dom_s2", "dom_s6", "dom_s12", "dom_s22g", "dom_s38g4",
            "dom_s2i", "dom_s6i", "dom_s12i", "dom_s22gi", "dom_s38g4i"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("env", "oa", "dom_off", "domains", "ops", "op_pp")


def shape_of(name):
    return int(re.match(r"dom_s(\d+)", name).group(1)), name.endswith("i")


def test_parametrisation_is_every_variant():
    assert VARIANTS == msv.Domain_HMM.variants()


class Profile:
    """A raw domain profile over a model's tables, forced to one variant.  msv_aln_describe is checked on entry: it
    reports R and neither null2 kernel spills."""

    def __init__(self, model, name):
        self.model, self.name = model, name

    def __enter__(self):
        self.p = decode_lib.create_profile(*self.model, self.name)
        info = _native.AlnInfo()
        assert _native.lib().msv_aln_describe(self.p, C.byref(info)) == 0
        self.info = info.as_dict()
        assert self.info["null2_row_block"] == R, self.info
        assert self.info["null2_partial_scratch_bytes"] == 0 and self.info["null2_finish_scratch_bytes"] == 0, self.info
        assert self.info["variant"] == self.name.replace("dom_", "aln_")
        return self

    def __exit__(self, *exc):
        decode_lib.destroy_profile(self.p)

    def run(self, codes, offsets, items, status=0, **kw):
        st, out = gpu_align_opts(self.p, self.model[0].shape[1], codes, offsets, items, **kw)
        assert st == status, _native.STATUS.get(st, st)
        return out


def test_describe_reports_the_row_block_and_no_scratch():
    for name in VARIANTS:
        S, isc = shape_of(name)
        with Profile(base_model(64 * S - 1, 3, isc), name) as p:
            for k in ("partial", "finish"):
                assert p.info[f"null2_{k}_scratch_bytes"] == 0 and p.info[f"null2_{k}_lds_bytes"] == 0
            old = _native.AlnInfo()
            old.struct_size = _native.AlnInfo.null2_row_block.offset  # a caller built before the fields were added
            assert _native.lib().msv_aln_describe(p.p, C.byref(old)) == 0
            assert old.null2_row_block == 0 and old.variant.decode() == p.info["variant"]


def check_null2(p, model, codes, offsets, items, bad, refs, what):
    """One device call with the posteriors kept on a list whose item `bad` holds a residue outside the 20; refs[q] =
    (null2, domcorrection) of msv_aln_cpu_null2.  Every item within the bounds of the module docstring, its
    domcorrection the definition on its own null2, its null2 the float64 sums over its own posteriors with the slots
    beyond the model left out; returns the result."""
    S, _ = shape_of(p.name)
    M = model[0].shape[1]
    leng = M - 1
    off = offsets.astype(np.int64)
    m32, i32 = odds32(model)
    out = p.run(codes, offsets, items, status=4, keep=True)
    assert out["null2"].shape == (len(items), 20) and out["null2_stats"]["row_block"] == R
    units = sum(-(-(b - a + 1) // R) for _, a, b in items)
    assert out["null2_stats"]["slab_bytes"] == units * (2 * S + 1) * 64 * 4 and out["stats"]["chunks"] == 1
    worst_n2 = worst_dc = worst_sum = worst_rows = 0.0
    for q, (s, a, b) in enumerate(items):
        Le = b - a + 1
        env = codes[off[s] + a - 1:off[s] + b]
        got, got_dc = out["null2"][q], out["domcorr"][q]
        if q == bad:
            assert out["env"][q] == np.inf and not got.any() and got_dc == 0.0
            continue
        ref, ref_dc = refs[q]
        delta = null2_bound(model, Le, ref)
        err = np.abs(got.astype(np.float64) - ref)
        worst_n2 = max(worst_n2, float(np.max(err / delta)))
        tol = domcorr_bound(env, ref, delta, ref_dc)
        worst_dc = max(worst_dc, abs(float(got_dc) - ref_dc) / tol)
        # the definition on the device's own null2: bit for bit
        st, want_dc = correction(got, env)
        assert st == 0 and bits(np.array([got_dc])) == bits(np.array([want_dc])), (what, q, got_dc, want_dc)
        # the masks at LENG and LENG - 1: float64 sums over the device's own posteriors, slots beyond the model
        # left out, insert column LENG (which msv_aln_result_posteriors hands over as the device left it) too
        pm, pi, pn, pj, pc = (x.astype(np.float64) for x in out["post"][q])
        eM, eI = pm.sum(axis=0), pi.sum(axis=0)
        eI[leng] = 0.0
        eX = float((pn + pj + pc).sum())
        total = eM.sum() + eI.sum() + eX
        worst_rows = max(worst_rows, abs(total - Le) / (Le * leng * float(post_bound(Le, leng))))
        own = (m32 @ eM + i32 @ eI + eX) / Le
        own_tol = 2.0 * (Le + 2.0 * leng + 8.0) * U * own  # the sums, the product, the scale: no posterior error
        worst_sum = max(worst_sum, float(np.max(np.abs(got.astype(np.float64) - own) / own_tol)))
    print(f"{what}: {len(items)} items; worst null2 error {worst_n2:.4f} of its bound, worst domcorrection "
          f"error {worst_dc:.4f} of its bound, null2 against float64 sums of the device's own posteriors "
          f"{worst_sum:.4f} of the summation bound, |sum_k (eM + eI) + eX - Le| {worst_rows:.2e} of Le LENG x the "
          f"posterior bound")
    assert worst_n2 <= 1.0 and worst_dc <= 1.0 and worst_sum <= 1.0 and worst_rows <= 1.0, what
    return out


@pytest.mark.parametrize("name", VARIANTS)
def test_null2_against_the_float64_twin(name):
    """LENG 64 S, 64 S - 1 and 64 (S - 2) + 1; null2_lib.null2_items: lane-edge homologs, envelopes of 1, 2, R - 1, R,
    R + 1, 2 R + 1 and 4 R + 3 residues, a cut from the middle of the longest, the first item again, a bad item."""
    S, isc = shape_of(name)
    for which in range(3):
        model, codes, offsets, items, bad, refs = case(S, isc, which)
        leng = model[0].shape[1] - 1
        what = f"{name} LENG {leng}"
        with Profile(model, name) as p:
            out = check_null2(p, model, codes, offsets, items, bad, refs, what)
            # the repeated item has its original's bytes; without the bad item the others keep theirs (a second call)
            rep = len(items) - 2
            assert out["null2"][rep].tobytes() == out["null2"][0].tobytes()
            assert out["domcorr"][rep].tobytes() == out["domcorr"][0].tobytes()
            clean = p.run(codes, offsets, items[:bad])
            assert clean["null2"].tobytes() == out["null2"][:bad].tobytes()
            assert clean["domcorr"].tobytes() == out["domcorr"][:bad].tobytes()


@pytest.mark.parametrize("name", VARIANTS)
def test_chunks_do_not_change_the_bytes(name):
    S, isc = shape_of(name)
    model, codes, offsets, items, bad, _ = case(S, isc, 1)
    items = items[:bad]
    nbytes = [int(_native.lib().msv_aln_item_bytes(S, b - a + 1)) for _, a, b in items]
    with Profile(model, name) as p:
        one = p.run(codes, offsets, items)
        assert one["stats"]["chunks"] == 1 and np.all(one["null2"] > 0)
        for ws in (max(nbytes), max(nbytes) + min(nbytes), 2 * max(nbytes)):
            cut = p.run(codes, offsets, items, workspace_bytes=ws)
            assert cut["stats"]["chunks"] > 1
            assert cut["null2_stats"]["slab_bytes"] < one["null2_stats"]["slab_bytes"]
            for f in FIELDS + ("null2", "domcorr"):
                assert cut[f].tobytes() == one[f].tobytes(), (ws, f)
        again = p.run(codes, offsets, items)
        assert again["null2"].tobytes() == one["null2"].tobytes()
        # an item's null2 does not depend on its place in the list
        back = p.run(codes, offsets, items[::-1])
        assert back["null2"][::-1].tobytes() == one["null2"].tobytes()
        assert back["domcorr"][::-1].tobytes() == one["domcorr"].tobytes()


def test_more_units_than_resident_waves():
    """4,099 sequences of a few residues at S = 2, their items repeated until the units outnumber the waves the device
    can hold at all (32 a compute unit: 8 a SIMD at the partial kernel's 27 VGPRs); the same items in small chunks give
    the same bytes."""
    import torch
    S, isc = 2, False
    model = base_model(64 * S, 91, isc)
    (codes, offsets), _ = queue_batch(model, 4099, 92)
    L = np.diff(offsets.astype(np.int64))
    once = [(s, 1, int(L[s])) for s in range(len(L)) if L[s] > 0]
    resident = 32 * torch.cuda.get_device_properties(0).multi_processor_count
    units_once = sum(-(-Le // R) for _, _, Le in once)
    items = once * (resident // units_once + 1)
    units = units_once * (len(items) // len(once))
    assert units > resident and len(items) > resident // 4  # more units than waves, more items than finish workgroups
    with Profile(model, "dom_s2") as p:
        deep = p.run(codes, offsets, items)
        assert deep["null2_stats"]["slab_bytes"] == units * (2 * S + 1) * 64 * 4 and deep["stats"]["chunks"] == 1
        first, last = deep["null2"][:len(once)], deep["null2"][-len(once):]
        assert first.tobytes() == last.tobytes()  # a repeated item has its original's bytes, wherever its units ran
        assert np.all(np.isfinite(deep["env"])) and np.all(deep["null2"] > 0) and np.all(np.isfinite(deep["domcorr"]))
        small = p.run(codes, offsets, items,
                      workspace_bytes=32 * int(_native.lib().msv_aln_item_bytes(S, int(L.max()))))
        assert small["stats"]["chunks"] > deep["stats"]["chunks"]
        for f in FIELDS + ("null2", "domcorr"):
            assert small[f].tobytes() == deep[f].tobytes(), f
        for q in (0, 1, len(items) // 2, len(items) - 1):
            s, a, b = items[q]
            st, want = correction(deep["null2"][q], codes[int(offsets[s]):int(offsets[s + 1])])
            assert st == 0 and bits(np.array([deep["domcorr"][q]])) == bits(np.array([want]))


def test_without_the_option_the_call_is_the_old_one():
    S, isc = 6, True
    model, codes, offsets, items, bad, _ = case(S, isc, 1)
    M = model[0].shape[1]
    with Profile(model, "dom_s6i") as p:
        st, old = align_lib.gpu_align(p.p, M, codes, offsets, items, keep=True)
        assert st == 4
        for options in (True, False):
            off_ = p.run(codes, offsets, items, status=4, keep=options, null2=False, options=options)
            assert off_["null2_status"] == 1 and "null2" not in off_
            for f in FIELDS:
                assert off_[f].tobytes() == old[f].tobytes(), f
            if options:
                for x, y in zip(off_["post"], old["post"]):
                    for u, v in zip(x, y):
                        assert u.tobytes() == v.tobytes()
        on = p.run(codes, offsets, items, status=4)
        for f in FIELDS:
            assert on[f].tobytes() == old[f].tobytes(), f
        ns = _native.AlnNull2Stats()
        assert _native.lib().msv_aln_result_null2(None, None, None) == 1
        assert _native.lib().msv_aln_result_null2_stats(None, C.byref(ns)) == 1


def test_search_pipeline_with_null2():
    """search_pipeline(align=True, null2=True) on a small batch with one planted low-complexity hit: a homolog whose
    tail is a run of one residue."""
    hmm = msv.Profile_HMM(os.path.join(ROOT, "data", "profile_HMMs", "1400.hmm"))
    engines = (msv.MSV_HMM(hmm, device=0), msv.Viterbi_HMM(hmm, device=0), msv.Forward_HMM(hmm, device=0))
    dom = msv.Domain_HMM(hmm, device=0)
    hom = homolog_batch(hmm.match_emissions, 23, 5, 250, 400)
    planted = np.concatenate([hom[0][int(hom[1][0]):int(hom[1][1])], np.full(60, 9, np.uint8)])
    codes, offsets = concat_batches(random_batch(3, 20, 300, 500), _csr([planted]), hom)
    planted_at = 20
    plain = msv.search_pipeline(*engines, codes=codes, offsets=offsets, dom_engine=dom, align=True)
    assert set(plain) == {"msv_scores", "passed_msv", "vit_scores", "passed_vit", "fwd_scores", "fwd_pvalues",
                          "envelopes", "alignments"}
    assert plain["alignments"].null2 is None and plain["alignments"].domcorrection is None
    with pytest.raises(ValueError):
        plain["alignments"].bias_scores(-3.0, 0.7)
    out = msv.search_pipeline(*engines, codes=codes, offsets=offsets, dom_engine=dom, align=True, null2=True)
    new = {"domain_bits", "domain_pvalues", "seq_bias", "seq_bits", "seq_pvalues"}
    assert set(out) == set(plain) | new
    aln, env = out["alignments"], out["envelopes"]
    hits = env.select.astype(np.int64)
    assert planted_at in hits and len(hits) >= 4 and len(aln) >= 4
    assert aln.null2.shape == (len(aln), 20) and np.all(aln.null2 > 0) and aln.stats["null2_row_block"] == R
    for f in ("envelope_scores", "oa_scores", "domains", "ops", "op_pp"):
        assert getattr(aln, f).tobytes() == getattr(plain["alignments"], f).tobytes(), f
    tau, lam = engines[2].forward_tau, engines[2].forward_lambda
    b = aln.bias_scores(tau, lam, fwd_scores=out["fwd_scores"])
    assert out["domain_bits"].tobytes() == b["domain_bits"].tobytes()
    assert out["domain_pvalues"].tobytes() == b["domain_pvalues"].tobytes()
    for k in ("seq_bias", "seq_bits", "seq_pvalues"):
        assert out[k].shape == (len(hits),) and out[k].tobytes() == b[k][hits].tobytes(), k
    # bias_scores is msv_aln_bias_scores on the same numbers, exactly
    lengths = np.diff(offsets.astype(np.int64))
    Le = aln.items["i_to"].astype(np.int64) - aln.items["i_from"].astype(np.int64) + 1
    st, want = null2_lib.bias_scores(aln.envelope_scores, Le, lengths[aln.items["seq"].astype(np.int64)],
                                     aln.domcorrection, tau, lam, aln.items["seq"], out["fwd_scores"], lengths)
    assert st == 0
    for k, v in want.items():
        assert v.tobytes() == b[k].tobytes(), k
    # each device domcorrection is the definition on the device's null2
    for q in range(len(aln)):
        s, a, e = (int(aln.items[f][q]) for f in ("seq", "i_from", "i_to"))
        st, dc = correction(aln.null2[q], codes[int(offsets[s]) + a - 1:int(offsets[s]) + e])
        assert st == 0 and bits(np.array([aln.domcorrection[q]])) == bits(np.array([dc]))
    # the planted sequence: corrected below uncorrected, and its P-value no smaller than Forward's own
    at = int(np.flatnonzero(hits == planted_at)[0])
    L = int(lengths[planted_at])
    p1 = np.float32(L) / np.float32(L + 1)
    nullsc = np.float32(L * np.log(np.float64(p1)) + np.log(1.0 - np.float64(p1)))
    uncorrected = np.float32(np.float32(out["fwd_scores"][planted_at] - nullsc) / np.float32(0.69314718055994529))
    assert out["seq_bits"][at] < uncorrected and out["seq_bias"][at] > 0
    # (that much holds for any finite correction.)  What the correction has to show here: the planted sequence's
    # envelopes are richer in the residues its aligned states favour than null1 says, so its summed correction is
    # positive and its bias exceeds log(1 + omega), the bias of a sequence whose null2 is flat
    planted_dc = float(aln.domcorrection[aln.items["seq"] == planted_at].astype(np.float64).sum())
    assert planted_dc > 0.0 and out["seq_bias"][at] > np.float32(np.log1p(1.0 / 256.0)), planted_dc
    assert out["seq_pvalues"][at] >= out["fwd_pvalues"][planted_at]
    print(f"planted: uncorrected {float(uncorrected):.3f} bits, corrected {float(out['seq_bits'][at]):.3f}, seq_bias "
          f"{float(out['seq_bias'][at]):.4f} nats; the hits' seq_bias {np.round(out['seq_bias'], 4)}")
    with pytest.raises(ValueError):
        msv.search_pipeline(*engines, codes=codes, offsets=offsets, dom_engine=dom, null2=True)
    with pytest.raises(ValueError):
        msv.search_pipeline(*engines, codes=codes, offsets=offsets, align=True, null2=True)
    dom.close()
