"""The alignment stage on the GPU (aln_kernel.hip), every variant: the recording Forward kernel with the
full matrix, Backward with the per-cell combine, the optimal-accuracy fill and the walk, against the library's CPU
functions on the same tables.

Bounds are msv.h's: every posterior |gpu - cpu64| <= 48 (Le + LENG) 2^-24 + 2 2^-24 absolute; the OA score within
Le (that bound) + Le^2 2^-24 of the float64 twin; the envelope score within Forward's bound, and with Lc = Le equal to
the Forward kernel's of the same variant bit for bit.  Paths have no tolerance: domains, ops, op_pp and the OA score
of the device equal msv_aln_oa run on the device's own posteriors, byte for byte.  The worst errors are printed before
they are asserted; DESIGN 4.11 records them."""
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import hmm_fasta_viterbi_amd as msv
from hmm_fasta_viterbi_amd import _native
from hmm_fasta_viterbi_amd.synthetic import concat_batches, random_batch
import ctypes as C

import align_lib
import decode_lib
import forward_lib
from align_lib import gpu_align, item_domains, oa_bound, post_bound
from forward_batches import aimed_batch, base_model, bridge_model, consensus, insertion_batch, queue_batch
from forward_lib import U
from oracle_lib import bits
from state_batches import _csr

VARIANTS = ["dom_s2", "dom_s6", "dom_s12", "dom_s22g", "dom_s38g4",
            "dom_s2i", "dom_s6i", "dom_s12i", "dom_s22gi", "dom_s38g4i"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OOM = 9


def shape_of(name):
    return int(re.match(r"dom_s(\d+)", name).group(1)), name.endswith("i")


def test_parametrisation_is_every_variant():
    assert VARIANTS == msv.Domain_HMM.variants()


class Profile:
    """A raw domain profile over a model's tables, forced to one variant.  msv_aln_describe is checked on entry: the
    alignment variant follows the profile's, and none of the four kernels spills."""

    def __init__(self, model, name):
        self.model, self.name = model, name

    def __enter__(self):
        S, isc = shape_of(self.name)
        self.p = decode_lib.create_profile(*self.model, self.name)
        info = _native.AlnInfo()
        assert _native.lib().msv_aln_describe(self.p, C.byref(info)) == 0
        self.info = info.as_dict()
        assert self.info["variant"] == self.name.replace("dom_", "aln_"), self.info
        assert self.info["states_per_lane"] == S and self.info["pointer_words"] == (S + 7) // 8
        for k in ("forward", "backward", "fill", "walk"):
            assert self.info[k + "_scratch_bytes"] == 0, self.info
        return self

    def __exit__(self, *exc):
        decode_lib.destroy_profile(self.p)

    def align(self, codes, offsets, items, **kw):
        st, out = gpu_align(self.p, self.model[0].shape[1], codes, offsets, items, **kw)
        assert st == 0, _native.STATUS.get(st, st)
        return out


def stretch(model, L, seed):
    """A sequence of exactly L residues made of consensus runs (every row carries mass)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    leng = model[0].shape[1] - 1
    parts, have = [], 0
    while have < L:
        core = min(20, leng, L - have)
        start = int(rng.integers(1, leng - core + 2))
        parts.append(consensus(model, start, start + core - 1))
        have += core
    return np.concatenate(parts)


def take(batch, idx):
    return _csr([batch[0][int(batch[1][i]):int(batch[1][i + 1])] for i in idx])


def edge_items(model, S):
    """The capacity-edge batch (every fourth tail and head homolog, every window), the insertion batch, envelopes of
    exactly 1, 2, 64, 65 and 129 residues; every non-empty sequence whole, then one envelope cut from the middle of
    the 129-residue sequence (i_from > 1, Lc > Le) and the first item again.  A model too short for the aimed batches
    (LENG < 24) has the fixed lengths and uniform sequences."""
    leng = model[0].shape[1] - 1
    blocks = _csr([stretch(model, L, 600 + L) for L in (1, 2, 64, 65, 129)])
    if leng >= 24:
        (aimed, where), (ins, _) = aimed_batch(model, S, 32), insertion_batch(model, S, 42)
        pick = np.concatenate([where["tail"][::4], where["head"][::4], where.get("window", np.zeros(0, np.int64))])
        batch = concat_batches(take(aimed, pick.astype(np.int64)), take(ins, range(0, len(ins[1]) - 1, 2)), blocks)
    else:
        batch = concat_batches(random_batch(33, 6, 1, 40), blocks)
    codes, offsets = batch
    n = len(offsets) - 1
    L = np.diff(offsets.astype(np.int64))
    items = [(s, 1, int(L[s])) for s in range(n) if L[s] > 0]
    items.append((n - 1, 20, 90))
    items.append(items[0])
    return codes, offsets, items


def check_items(p, codes, offsets, items, what, forward_bits=False):
    """One device call with the posteriors kept, every check of the module docstring; returns the result."""
    model = p.model
    M = model[0].shape[1]
    leng = M - 1
    out = p.align(codes, offsets, items, keep=True)
    assert out["stats"]["chunks"] >= 1 and len(out["env"]) == len(items)
    off = offsets.astype(np.int64)
    worst_pp = worst_row = worst_oa = worst_env = 0.0
    for q, (s, a, b) in enumerate(items):
        Le, Lc = b - a + 1, int(off[s + 1] - off[s])
        env_codes = codes[off[s] + a - 1:off[s] + b]
        st, score, *ref = align_lib.cpu_decode(model, env_codes, Lc)
        assert st == 0
        post = out["post"][q]
        bound = float(post_bound(Le, leng))
        for name, g, w in zip(("ppM", "ppI", "ppN", "ppJ", "ppC"), post, ref):
            err = float(np.max(np.abs(g.astype(np.float64) - w)))
            worst_pp = max(worst_pp, err / bound)
            assert err <= bound, (what, q, name, err, bound)
        rows = sum(x.astype(np.float64).sum(axis=1) for x in post[:2]) + sum(x.astype(np.float64) for x in post[2:])
        row_err = float(np.max(np.abs(rows - 1.0)))
        worst_row = max(worst_row, row_err / (leng * bound))
        assert row_err <= leng * bound, (what, q, row_err)
        env_tol = float(forward_lib.tolerance(Le, leng, score))
        worst_env = max(worst_env, abs(float(out["env"][q]) - score) / env_tol)
        assert abs(float(out["env"][q]) - score) <= env_tol, (what, q, out["env"][q], score)
        # exactness: the definition on the device's own posteriors
        want_oa, wd, wo, wp = msv.aln_oa(*post, model[2], model[3], Lc)
        gd, go, gp = item_domains(out, q)
        wd = wd.copy()
        wd["seq"] = s
        wd["i_from"] += a - 1
        wd["i_to"] += a - 1
        assert bits(np.array([out["oa"][q]])) == bits(np.array([want_oa])), (what, q, out["oa"][q], want_oa)
        assert gd.tobytes() == wd.tobytes(), (what, q, gd, wd)
        assert go.tobytes() == wo.tobytes() and gp.tobytes() == wp.tobytes(), (what, q)
        # the OA score against the float64 twin
        st, _, twin_oa, *_ = align_lib.cpu_align(model, env_codes, Lc)
        assert st == 0
        ob = float(oa_bound(Le, leng))
        worst_oa = max(worst_oa, abs(float(out["oa"][q]) - float(twin_oa)) / ob)
        assert abs(float(out["oa"][q]) - float(twin_oa)) <= ob, (what, q, out["oa"][q], twin_oa)
    print(f"{what}: {len(items)} items; worst posterior error {worst_pp:.4f} of its bound, worst row sum "
          f"{worst_row:.2e} of LENG x bound, worst OA score error {worst_oa:.2e} of its bound, worst envelope score "
          f"error {worst_env:.4f} of Forward's bound")
    if forward_bits:
        whole = [q for q, (s, a, b) in enumerate(items) if a == 1 and b == off[s + 1] - off[s]]
        sub = _csr([codes[off[items[q][0]]:off[items[q][0] + 1]] for q in whole])
        f = forward_lib.create_profile(*model, p.name.replace("dom_", "fwd_"))
        try:
            st, want = forward_lib.gpu_scores(f, *sub)
            assert st == 0
        finally:
            forward_lib.destroy_profile(f)
        assert np.array_equal(bits(out["env"][whole]), bits(want)), what
    return out


@pytest.mark.parametrize("name", VARIANTS)
def test_capacity_edges(name):
    """LENG 64 S, 64 S - 1 and 64 (S - 2) + 1."""
    S, isc = shape_of(name)
    for short, leng in enumerate((64 * S, 64 * S - 1, 64 * (S - 2) + 1)):
        model = base_model(leng, 31 + short, isc)
        codes, offsets, items = edge_items(model, S)
        with Profile(model, name) as p:
            out = check_items(p, codes, offsets, items, f"capacity edges {name} LENG {leng}", forward_bits=True)
            if short == 0:
                # sum_k (ppM + ppI) is occ, counted on the core states: against the decode's own occ (Lc = Le items)
                st, env = decode_lib.gpu_decode(p.p, codes, offsets)
                assert st == 0
                worst = 0.0
                for q, (s, a, b) in enumerate(items[:-2]):
                    pm, pi = out["post"][q][:2]
                    core = pm.astype(np.float64).sum(axis=1) + pi.astype(np.float64).sum(axis=1)
                    Le = b - a + 1
                    tol = float(leng * post_bound(Le, leng) + decode_lib.post_tolerance(Le, leng))
                    err = float(np.max(np.abs(core - env.posteriors(s)[2])))
                    worst = max(worst, err)
                    assert err <= tol, (q, err, tol)
                print(f"{name}: worst |sum_k (ppM + ppI) - occ| = {worst:.3e}")
            # the cut item is its parent's rows under another configured length, the repeat its original
            assert np.array_equal(bits(out["oa"][-1:]), bits(out["oa"][:1]))
            assert item_domains(out, len(items) - 1)[0].tobytes() == item_domains(out, 0)[0].tobytes()
            cut = item_domains(out, len(items) - 2)[0]
            assert np.all(cut["i_from"] >= 20) and np.all(cut["i_to"] <= 90) and np.all(cut["seq"] == items[-2][0])


@pytest.mark.parametrize("name", VARIANTS)
def test_bridges(name):
    """bridge_model: the aligned path of each bridge sequence deletes across more lanes than a scan step covers."""
    from test_gpu_forward_boundaries import bridge_plain
    S, isc = shape_of(name)
    model = bridge_model(S, 11, isc)
    codes, offsets = bridge_plain(model, S)
    L = np.diff(offsets.astype(np.int64))
    items = [(s, 1, int(L[s])) for s in range(len(L))]
    with Profile(model, name) as p:
        out = check_items(p, codes, offsets, items, f"bridges {name}")
        runs = [max(len(r) for r in item_domains(out, q)[1].tobytes().replace(b"I", b"M").split(b"M"))
                for q in range(len(items))]
        assert max(runs) > 32 * S  # a D run across more than 32 lanes: the scan's last step carried it
    # one more bridge across each of the boundaries of lanes 1, 16, 32 and 63 (test_align_batches.py shows they cross)
    from forward_batches import BOUNDARY_LANES
    from test_align_batches import boundary_bridge
    for lane in BOUNDARY_LANES:
        bridged, seq, b = boundary_bridge(model, S, lane)
        with Profile(bridged, name) as p:
            check_items(p, *_csr([seq]), [(0, 1, len(seq))], f"bridge across lane {lane}'s boundary, {name}")


@pytest.mark.parametrize("name", VARIANTS)
def test_chunks_do_not_change_the_bytes(name):
    S, isc = shape_of(name)
    model = base_model(64 * S - 1, 32, isc)
    codes, offsets, items = edge_items(model, S)
    items = items[-12:]
    nbytes = [int(_native.lib().msv_aln_item_bytes(S, b - a + 1)) for _, a, b in items]
    with Profile(model, name) as p:
        one = p.align(codes, offsets, items, keep=False)
        assert one["stats"]["chunks"] == 1
        for ws in (max(nbytes), max(nbytes) + min(nbytes)):
            cut = p.align(codes, offsets, items, keep=False, workspace_bytes=ws)
            assert cut["stats"]["chunks"] > 1
            for f in ("env", "oa", "dom_off", "domains", "ops", "op_pp"):
                assert cut[f].tobytes() == one[f].tobytes(), (ws, f)
        st, refused = gpu_align(p.p, model[0].shape[1], codes, offsets, items, workspace_bytes=max(nbytes) - 1,
                                keep=False)
        assert st == OOM and refused["stats"]["chunks"] == 0 and len(refused["domains"]) == 0


@pytest.mark.parametrize("name", VARIANTS)
def test_more_items_than_resident_waves(name):
    """4,099 short items: every wave takes several; the same items run in chunks of a few give the same bytes."""
    S, isc = shape_of(name)
    model = base_model(64 * S, 91, isc)
    (codes, offsets), chains = queue_batch(model, 4099, 92)
    L = np.diff(offsets.astype(np.int64))
    items = [(s, 1, int(L[s])) for s in range(len(L)) if L[s] > 0]
    with Profile(model, name) as p:
        deep = p.align(codes, offsets, items, keep=False)
        assert np.all(np.isfinite(deep["env"])) and np.diff(deep["dom_off"].astype(np.int64)).max() >= 2
        small = p.align(codes, offsets, items, keep=False,
                        workspace_bytes=8 * int(_native.lib().msv_aln_item_bytes(S, int(L.max()))))
        assert small["stats"]["chunks"] > deep["stats"]["chunks"]
        for f in ("env", "oa", "dom_off", "domains", "ops", "op_pp"):
            assert small[f].tobytes() == deep[f].tobytes(), f
        again = p.align(codes, offsets, items, keep=False)  # the counters were reset by the last workgroup to leave
        assert again["ops"].tobytes() == deep["ops"].tobytes()


SHARED_LENGTHS = (30, 47, 80, 64, 55)
# two overlapping items on sequence 3, one of a single residue, two whole sequences; not in sequence order
SHARED_ITEMS = [(3, 10, 50), (0, 1, 30), (3, 30, 64), (1, 17, 17), (4, 5, 40), (2, 1, 80)]


def shared_batch(isc):
    """100.hmm's tables, five sequences of 30 to 80 residues and SHARED_ITEMS on them."""
    hmm = msv.Profile_HMM(os.path.join(ROOT, "data", "profile_HMMs", "100.hmm"))
    model = forward_lib.tables(hmm, 1 if isc else 0)
    codes, offsets = _csr([stretch(model, L, 800 + L) for L in SHARED_LENGTHS])
    return model, codes, offsets, list(SHARED_ITEMS)


@pytest.mark.parametrize("name", VARIANTS)
def test_item_order_and_shared_sequences(name):
    """An item's bytes do not depend on the items around it: each of SHARED_ITEMS alone against one call over all of
    them whose workspace holds two of the largest, so that the call runs in several chunks."""
    S, isc = shape_of(name)
    model, codes, offsets, items = shared_batch(isc)
    nbytes = [int(_native.lib().msv_aln_item_bytes(S, b - a + 1)) for _, a, b in items]
    with Profile(model, name) as p:
        batch = p.align(codes, offsets, items, keep=False, workspace_bytes=2 * max(nbytes))
        assert batch["stats"]["chunks"] > 1 and len(batch["env"]) == len(items)
        assert np.all(np.isfinite(batch["env"])) and len(batch["domains"]) >= 1
        for q, item in enumerate(items):
            alone = p.align(codes, offsets, [item], keep=False)
            assert alone["stats"]["chunks"] == 1
            assert bits(batch["env"][q:q + 1]) == bits(alone["env"]), (q, item)
            assert bits(batch["oa"][q:q + 1]) == bits(alone["oa"]), (q, item)
            for x, y in zip(item_domains(batch, q), item_domains(alone, 0)):
                assert x.tobytes() == y.tobytes(), (q, item)


def test_error_classes():
    S, isc = 6, False
    model = base_model(64 * S, 31, isc)
    seqs = [stretch(model, L, 700 + L) for L in (40, 70, 30)]
    codes, offsets = _csr(seqs)
    items = [(0, 1, 40), (1, 10, 60), (2, 1, 30), (1, 1, 9)]
    with Profile(model, "dom_s6") as p:
        good = p.align(codes, offsets, items)
        bad = codes.copy()
        bad[int(offsets[1]) + 30] = 21  # inside item 1, outside item 3
        st, out = gpu_align(p.p, model[0].shape[1], bad, offsets, items)
        assert st == 4 and out["env"][1] == np.inf and out["dom_off"][2] == out["dom_off"][1]
        for q in (0, 2, 3):
            assert bits(out["env"][q:q + 1]) == bits(good["env"][q:q + 1])
            for x, y in zip(item_domains(out, q), item_domains(good, q)):
                assert x.tobytes() == y.tobytes()
        outside = codes.copy()
        outside[int(offsets[1]) + 65] = 21  # in sequence 1, in no item
        st, out = gpu_align(p.p, model[0].shape[1], outside, offsets, items)
        assert st == 0 and out["ops"].tobytes() == good["ops"].tobytes()
        again = p.align(codes, offsets, items)  # the error word was cleared
        assert again["ops"].tobytes() == good["ops"].tobytes()
        for wrong in ((3, 1, 5), (0, 0, 5), (0, 5, 4), (0, 1, 41)):
            st, out = gpu_align(p.p, model[0].shape[1], codes, offsets, [wrong])
            assert st == 1 and out is None


def test_python_engine_and_search_pipeline():
    """Domain_HMM.align_batch as a user holds it, and search_pipeline(align=True) against align_batch by hand."""
    from hmm_fasta_viterbi_amd.synthetic import homolog_batch
    hmm = msv.Profile_HMM(os.path.join(ROOT, "data", "profile_HMMs", "1400.hmm"))
    engines = (msv.MSV_HMM(hmm, device=0), msv.Viterbi_HMM(hmm, device=0), msv.Forward_HMM(hmm, device=0))
    dom = msv.Domain_HMM(hmm, device=0)
    codes, offsets = concat_batches(random_batch(2, 56, 300, 500), homolog_batch(hmm.match_emissions, 21, 8, 250, 400))
    plain = msv.search_pipeline(*engines, codes=codes, offsets=offsets, dom_engine=dom)
    assert set(plain) == {"msv_scores", "passed_msv", "vit_scores", "passed_vit", "fwd_scores", "fwd_pvalues",
                          "envelopes"}
    out = msv.search_pipeline(*engines, codes=codes, offsets=offsets, dom_engine=dom, align=True)
    assert set(out) == set(plain) | {"alignments"}
    aln, env = out["alignments"], out["envelopes"]
    assert len(aln) == len(env.regions) >= 4 and aln.status == "MSV_OK"
    hand = dom.align_batch(codes=codes, offsets=offsets,
                           items=[(int(r["seq"]), int(r["i_from"]), int(r["i_to"])) for r in env.regions],
                           keep_posteriors=True)
    for f in ("envelope_scores", "domain_scores", "oa_scores", "accuracy", "domain_offsets", "domains", "ops", "op_pp"):
        assert getattr(hand, f).tobytes() == getattr(aln, f).tobytes(), f
    leng = hmm.model_length - 1
    for q in range(len(aln)):
        r = env.regions[q]
        Le = int(r["i_to"]) - int(r["i_from"]) + 1
        lo = int(offsets[int(r["seq"])])
        Lc = int(offsets[int(r["seq"]) + 1]) - lo
        sc, oa, doms, ops, pp = dom.align_on_sequence(codes=codes[lo + int(r["i_from"]) - 1:lo + int(r["i_to"])], Lc=Lc)
        assert abs(float(aln.envelope_scores[q]) - sc) <= forward_lib.tolerance(Le, leng, sc)
        assert abs(float(aln.oa_scores[q]) - float(oa)) <= oa_bound(Le, leng)
        assert 0.5 < aln.accuracy[q] <= 1.0 + Le * U and aln.domain_scores[q] < aln.envelope_scores[q]
        d = aln.domains_of(q)
        assert len(d) >= 1 and np.all(d["seq"] == r["seq"]) and d["i_from"].min() >= r["i_from"]
        line = aln.pp_line(d[0])
        assert len(line) == int(d[0]["ops_len"])
        for ch, op, pr in zip(line, aln.ops_of(d[0]), aln.pp_of(d[0])):
            assert ch == ("." if op == 68 else "*" if float(pr) + 0.05 >= 1.0 else str(int(10.0 * float(pr) + 0.5)))
        want = msv.aln_oa(*hand.posteriors(q), dom.transition_scores, (dom.tr_B_Mk, dom.tr_E_C, dom.tr_E_J), Lc)
        assert hand.ops_of(d[0]) == want[2][:int(d[0]["ops_len"])].tobytes()
    with pytest.raises(ValueError):
        msv.search_pipeline(*engines, codes=codes, offsets=offsets, align=True)
    dom.close()
