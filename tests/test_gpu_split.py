"""The split stage on the GPU (spl_kernel.hip), every variant: the recording Forward launch that keeps fM,
fI and fD, and the stochastic traceback sampler, against the library's CPU functions on the same tables.

Bounds are msv.h's: every recorded f, once its row's exponent is applied, within the relative 16 (Le + LENG) 2^-24 of
the float64 twin msv_spl_cpu_forward (absolute 2^-126 in the row's scale where the float32 value is subnormal or zero);
the envelope score within Forward's bound, with Lc = Le equal to the Forward kernel's of the same variant and to the
alignment stage's recording launch bit for bit (the alignment stage exposes no fM download: its planes become
posteriors in place, so fM / fI / fD are held to the twin).  Samples have no tolerance: every item's segments equal
msv_spl_sample run on the host over the downloaded matrix, byte for byte, and no sample is truncated.  The worst share
of the bound is printed before it is asserted; DESIGN 4.14 records it."""
import ctypes as C
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import hmm_fasta_viterbi_amd as msv
from hmm_fasta_viterbi_amd import _native
from hmm_fasta_viterbi_amd.synthetic import concat_batches, random_batch

import decode_lib
import forward_lib
import split_lib
from align_lib import gpu_align
from forward_batches import base_model, queue_batch
from oracle_lib import bits
from split_lib import (DRAWS, PLAN, cpu_forward, draws_on_rescaled_rows, f_bound, gpu_batches, gpu_model, gpu_sample,
                       host_segments, item_segments)
from state_batches import _csr
from test_gpu_align import stretch

VARIANTS = ["dom_s2", "dom_s6", "dom_s12", "dom_s22g", "dom_s38g4",
            "dom_s2i", "dom_s6i", "dom_s12i", "dom_s22gi", "dom_s38g4i"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OOM = 9
NS = 65  # an item's samples cross a wave


def shape_of(name):
    return int(re.match(r"dom_s(\d+)", name).group(1)), name.endswith("i")


def test_parametrisation_is_every_variant():
    """Every domain variant has its split variant (msv_spl_describe), and VARIANTS is all of them."""
    assert VARIANTS == msv.Domain_HMM.variants()
    for name in VARIANTS:
        S, isc = shape_of(name)
        with Profile(base_model(64 * S, 30, isc), name) as p:
            assert p.info["variant"] == name.replace("dom_", "spl_")


class Profile:
    """A raw domain profile over a model's tables, forced to one variant.  msv_spl_describe is checked on entry: the
    split variant follows the profile's, and neither new kernel spills."""

    def __init__(self, model, name):
        self.model, self.name = model, name

    def __enter__(self):
        S, isc = shape_of(self.name)
        self.p = decode_lib.create_profile(*self.model, self.name)
        info = _native.SplInfo()
        assert _native.lib().msv_spl_describe(self.p, C.byref(info)) == 0
        self.info = info.as_dict()
        assert self.info["variant"] == self.name.replace("dom_", "spl_"), self.info
        assert self.info["states_per_lane"] == S
        assert self.info["forward_scratch_bytes"] == 0 and self.info["sample_scratch_bytes"] == 0, self.info
        return self

    def __exit__(self, *exc):
        decode_lib.destroy_profile(self.p)

    def sample(self, codes, offsets, items, **kw):
        st, out = gpu_sample(self.p, self.model[0].shape[1], codes, offsets, items, NS, **kw)
        assert st == 0, _native.STATUS.get(st, st)
        return out


def edge_items(S, isc, which):
    """The model split_lib.gpu_model(S, isc, which) and its items: where split_lib.PLAN has an entry (the model has
    the nodes for a copy) the strong homolog, the two-copy sequence and its control of that entry -- the batches
    tests/test_split_batches.py weighs on the CPU twin --, then envelopes of exactly 1, 2, 64, 65 and 129 residues;
    every sequence whole, then one envelope cut from the middle of the 129-residue sequence (i_from > 1, Lc > Le) and
    the first item again.  Returns (model, codes, offsets, items, index of the strong homolog's item or None)."""
    seqs, strong = [], None
    if (S, isc, which) in PLAN:
        model, ((cc, co), _, _), homolog = gpu_batches(S, isc, which)
        # (the homolog first: its samples are keyed by sequence 0, as the twin's are in test_split_batches.py)
        seqs += [homolog, cc[int(co[0]):int(co[1])], cc[int(co[1]):int(co[2])]]
        strong = 0
    else:
        model = gpu_model(S, isc, which)
    seqs += [stretch(model, L, 600 + L) for L in (1, 2, 64, 65, 129)]
    codes, offsets = _csr(seqs)
    L = np.diff(offsets.astype(np.int64))
    n = len(L)
    items = [(s, 1, int(L[s])) for s in range(n)]
    items.append((n - 1, 20, 90))
    items.append(items[0])
    return model, codes, offsets, items, strong


def check_items(p, codes, offsets, items, what, strong=None):
    """One device call with the matrix kept, every check of the module docstring; returns the result."""
    model = p.model
    M = model[0].shape[1]
    leng = M - 1
    out = p.sample(codes, offsets, items, keep=True)
    assert out["stats"]["chunks"] >= 1 and len(out["env"]) == len(items)
    assert out["stats"]["truncated"] == 0 and out["stats"]["n_samples"] == NS and out["stats"]["seed"] == split_lib.SEED
    off = offsets.astype(np.int64)
    worst_f = worst_env = 0.0
    rescaled = 0
    for q, (s, a, b) in enumerate(items):
        Le, Lc = b - a + 1, int(off[s + 1] - off[s])
        env_codes = codes[off[s] + a - 1:off[s] + b]
        st, score, fm, fi, fd, sp, ex = cpu_forward(model, env_codes, Lc)
        assert st == 0
        gm, gi, gd, rec = out["mat"][q]
        ge = rec[:, 5].view(np.int32).astype(np.int64)
        assert ge[0] == 0 and np.all(np.diff(ge) >= 0)
        rescaled += int(ge[-1] > 0)
        bound = f_bound(Le, leng)
        shift = (ex.astype(np.int64) - ge).astype(np.int32)
        pairs = [(g, np.ldexp(w, shift[1:, None])) for g, w in ((gm, fm), (gi, fi), (gd, fd))]
        pairs.append((rec[:, :5].view(np.float32), np.ldexp(sp, shift[:, None])))
        for g, w in pairs:
            g64 = g.astype(np.float64)
            err = np.abs(g64 - w)
            normal = np.abs(g64) >= 2.0 ** -126
            if normal.any():
                share = float(np.max(err[normal] / np.abs(w[normal]))) / bound
                worst_f = max(worst_f, share)
                assert share <= 1.0, (what, q, share)
            assert np.all(err[~normal] < 2.0 ** -126), (what, q)
        env_tol = float(forward_lib.tolerance(Le, leng, score))
        worst_env = max(worst_env, abs(float(out["env"][q]) - score) / env_tol)
        assert abs(float(out["env"][q]) - score) <= env_tol, (what, q, out["env"][q], score)
        # exactness: the definition on the device's own matrix
        want_n, want_segs, trunc = host_segments(model, out["mat"][q], Lc, s, a, b, NS)
        got_n, got_segs = item_segments(out, q, NS)
        assert trunc == 0
        assert np.array_equal(got_n, want_n), (what, q)
        assert got_segs.tobytes() == want_segs.tobytes(), (what, q)
        assert len(got_segs) == 0 or (got_segs["i_from"].min() >= a and got_segs["i_to"].max() <= b)
        if q == strong:
            # the strong homolog rescales several times, and some sample takes each special draw on a row whose
            # recorded exponent differs from the row before (tests/test_split_batches.py: so does the twin)
            assert ge[-1] >= 96 and np.count_nonzero(np.diff(ge)) >= 3, (what, ge[-1])
            cuts = np.cumsum(got_n)
            met = draws_on_rescaled_rows(rec, np.split(got_segs, cuts[:-1]), a)
            print(f"{what}: the strong homolog rescales on {np.count_nonzero(np.diff(ge))} rows; samples that meet "
                  f"one: {met}")
            for k in DRAWS:
                assert met[k] >= 1, (what, k, met)
    print(f"{what}: {len(items)} items x {NS} samples, {len(out['segments'])} segments, {rescaled} items rescaled; "
          f"worst f error {worst_f:.4f} of its bound, worst envelope score error {worst_env:.4f} of Forward's bound")
    return out


@pytest.mark.parametrize("name", VARIANTS)
def test_capacity_edges(name):
    """LENG 64 S, 64 S - 1 and 64 (S - 2) + 1."""
    S, isc = shape_of(name)
    for short, leng in enumerate((64 * S, 64 * S - 1, 64 * (S - 2) + 1)):
        model, codes, offsets, items, strong = edge_items(S, isc, short)
        assert model[0].shape[1] - 1 == leng
        off = offsets.astype(np.int64)
        with Profile(model, name) as p:
            out = check_items(p, codes, offsets, items, f"split capacity edges {name} LENG {leng}", strong)
            # the envelope scores are the alignment stage's recording launch's, and with Lc = Le the Forward kernel's
            st, aln = gpu_align(p.p, model[0].shape[1], codes, offsets, items, keep=False)
            assert st == 0 and np.array_equal(bits(out["env"]), bits(aln["env"]))
            whole = [q for q, (s, a, b) in enumerate(items) if a == 1 and b == off[s + 1] - off[s]]
            sub = _csr([codes[off[items[q][0]]:off[items[q][0] + 1]] for q in whole])
            f = forward_lib.create_profile(*model, name.replace("dom_", "fwd_"))
            try:
                st, want = forward_lib.gpu_scores(f, *sub)
                assert st == 0
            finally:
                forward_lib.destroy_profile(f)
            assert np.array_equal(bits(out["env"][whole]), bits(want))
            # the repeat is its original; the cut item stays inside its envelope, keyed by its own identity
            first, last = item_segments(out, 0, NS), item_segments(out, len(items) - 1, NS)
            assert np.array_equal(first[0], last[0]) and first[1].tobytes() == last[1].tobytes()
            cut = item_segments(out, len(items) - 2, NS)[1]
            assert len(cut) and np.all(cut["i_from"] >= 20) and np.all(cut["i_to"] <= 90)
            if strong is not None:
                # the two-copy sequence whole: two clusters; the control: one
                two = msv.spl_cluster(item_segments(out, 1, NS)[1], NS)
                one = msv.spl_cluster(item_segments(out, 2, NS)[1], NS)
                assert len(two) == 2 and len(one) == 1, (two, one)


@pytest.mark.parametrize("name", VARIANTS)
def test_layouts_do_not_change_the_bytes(name):
    """Another item order, a workspace of two items, of exactly the largest item, a second stream: an item's bytes
    stay.  One byte less than the largest item needs is refused before any launch."""
    import torch
    S, isc = shape_of(name)
    model, codes, offsets, items, _ = edge_items(S, isc, 1)  # LENG 64 S - 1
    items = items[-8:]
    nbytes = [int(_native.lib().msv_spl_item_bytes(S, b - a + 1)) for _, a, b in items]
    with Profile(model, name) as p:
        one = p.sample(codes, offsets, items)
        assert one["stats"]["chunks"] == 1 and one["stats"]["truncated"] == 0
        for ws in (max(nbytes), max(nbytes) + min(nbytes), 2 * max(nbytes)):
            cut = p.sample(codes, offsets, items, workspace_bytes=ws)
            assert cut["stats"]["chunks"] > 1
            for f in ("env", "sample_off", "segments"):
                assert cut[f].tobytes() == one[f].tobytes(), (ws, f)
        order = list(range(len(items)))[::-1]
        back = p.sample(codes, offsets, [items[q] for q in order])
        for j, q in enumerate(order):
            x, y = item_segments(back, j, NS), item_segments(one, q, NS)
            assert np.array_equal(x[0], y[0]) and x[1].tobytes() == y[1].tobytes(), q
            assert bits(back["env"][j:j + 1]) == bits(one["env"][q:q + 1])
        stream = torch.cuda.Stream()
        other = p.sample(codes, offsets, items, stream=stream.cuda_stream)
        stream.synchronize()
        for f in ("env", "sample_off", "segments"):
            assert other[f].tobytes() == one[f].tobytes(), f
        st, refused = gpu_sample(p.p, model[0].shape[1], codes, offsets, items, NS, workspace_bytes=max(nbytes) - 1)
        assert st == OOM and refused["stats"]["chunks"] == 0 and len(refused["segments"]) == 0


@pytest.mark.parametrize("name", VARIANTS)
def test_more_items_than_resident_waves(name):
    """4,099 short items: every wave takes several; the same items run in chunks of a few give the same bytes."""
    S, isc = shape_of(name)
    model = base_model(64 * S, 91, isc)
    (codes, offsets), chains = queue_batch(model, 4099, 92)
    L = np.diff(offsets.astype(np.int64))
    items = [(s, 1, int(L[s])) for s in range(len(L)) if L[s] > 0]
    with Profile(model, name) as p:
        deep = p.sample(codes, offsets, items)
        assert np.all(np.isfinite(deep["env"])) and deep["stats"]["truncated"] == 0
        assert np.diff(deep["sample_off"].astype(np.int64)).max() >= 2  # some sample has two domains
        small = p.sample(codes, offsets, items,
                         workspace_bytes=8 * int(_native.lib().msv_spl_item_bytes(S, int(L.max()))))
        assert small["stats"]["chunks"] > deep["stats"]["chunks"]
        for f in ("env", "sample_off", "segments"):
            assert small[f].tobytes() == deep[f].tobytes(), f
        # a few of them against the definition on their own matrices
        pick = [items[q] for q in (0, len(items) // 2, len(items) - 1)] + [items[int(chains[0])]]
        check_items(p, codes, offsets, pick, f"split deep queue {name}")


@pytest.mark.parametrize("name", VARIANTS)
def test_item_order_and_shared_sequences(name):
    """An item's bytes do not depend on the items around it: each of test_gpu_align's SHARED_ITEMS alone against one
    call over all of them, same seed, whose workspace holds two of the largest, so that it runs in several chunks."""
    from test_gpu_align import shared_batch
    S, isc = shape_of(name)
    model, codes, offsets, items = shared_batch(isc)
    nbytes = [int(_native.lib().msv_spl_item_bytes(S, b - a + 1)) for _, a, b in items]
    with Profile(model, name) as p:
        batch = p.sample(codes, offsets, items, workspace_bytes=2 * max(nbytes))
        assert batch["stats"]["chunks"] > 1 and len(batch["env"]) == len(items)
        assert np.all(np.isfinite(batch["env"])) and len(batch["segments"]) >= 1
        for q, item in enumerate(items):
            alone = p.sample(codes, offsets, [item])
            assert alone["stats"]["chunks"] == 1
            assert bits(batch["env"][q:q + 1]) == bits(alone["env"]), (q, item)
            x, y = item_segments(batch, q, NS), item_segments(alone, 0, NS)
            assert np.array_equal(x[0], y[0]) and x[1].tobytes() == y[1].tobytes(), (q, item)


def test_error_classes():
    S, isc = 6, False
    model = base_model(64 * S, 31, isc)
    seqs = [stretch(model, L, 700 + L) for L in (40, 70, 30)]
    codes, offsets = _csr(seqs)
    items = [(0, 1, 40), (1, 10, 60), (2, 1, 30), (1, 1, 9)]
    with Profile(model, "dom_s6") as p:
        good = p.sample(codes, offsets, items)
        bad = codes.copy()
        bad[int(offsets[1]) + 30] = 21  # inside item 1, outside item 3
        st, out = gpu_sample(p.p, model[0].shape[1], bad, offsets, items, NS)
        assert st == 4 and out["env"][1] == np.inf and len(item_segments(out, 1, NS)[1]) == 0
        for q in (0, 2, 3):
            assert item_segments(out, q, NS)[1].tobytes() == item_segments(good, q, NS)[1].tobytes()
        again = p.sample(codes, offsets, items)  # the error word was cleared
        assert again["segments"].tobytes() == good["segments"].tobytes()
        other_seed = gpu_sample(p.p, model[0].shape[1], codes, offsets, items, NS, seed=43)[1]
        assert other_seed["segments"].tobytes() != good["segments"].tobytes()
        for wrong in ((3, 1, 5), (0, 0, 5), (0, 5, 4), (0, 1, 41)):
            st, out = gpu_sample(p.p, model[0].shape[1], codes, offsets, [wrong], NS)
            assert st == 1 and out is None


def test_python_engine_and_search_pipeline():
    """Domain_HMM.sample_batch / split_regions as a user holds them, and search_pipeline(split=True): a two-copy
    homolog's region is aligned as two items, each with its own domain_bits; split=False returns what the call
    returns today, byte for byte."""
    hmm = msv.Profile_HMM(os.path.join(ROOT, "data", "profile_HMMs", "100.hmm"))
    engines = (msv.MSV_HMM(hmm, device=0), msv.Viterbi_HMM(hmm, device=0), msv.Forward_HMM(hmm, device=0))
    dom = msv.Domain_HMM(hmm, device=0)
    model = forward_lib.tables(hmm)
    (cc, co), planted, cores = split_lib.copies_batch(model)
    (c2, o2), _, _ = split_lib.copies_batch(model, seed=911)
    codes, offsets = concat_batches(random_batch(2, 24, 100, 200), (cc, co), (c2, o2))
    two_copy = [24, 26]
    assert dom.split_describe()["sample_scratch_bytes"] == 0

    today = msv.search_pipeline(*engines, codes=codes, offsets=offsets, dom_engine=dom, align=True, null2=True)
    plain = msv.search_pipeline(*engines, codes=codes, offsets=offsets, dom_engine=dom, align=True, null2=True,
                                split=False)
    assert set(plain) == set(today)
    for k, v in today.items():
        if isinstance(v, np.ndarray):
            assert plain[k].tobytes() == v.tobytes(), k
    for f in ("items", "envelope_scores", "domain_scores", "oa_scores", "domain_offsets", "domains", "ops", "op_pp",
              "null2", "domcorrection"):
        assert getattr(plain["alignments"], f).tobytes() == getattr(today["alignments"], f).tobytes(), f
    for f in ("forward_scores", "begin", "end", "occ", "regions", "region_offsets"):
        assert getattr(plain["envelopes"], f).tobytes() == getattr(today["envelopes"], f).tobytes(), f

    out = msv.search_pipeline(*engines, codes=codes, offsets=offsets, dom_engine=dom, align=True, null2=True, split=True)
    assert set(out) == set(today) | {"split"}
    env, aln, split = out["envelopes"], out["alignments"], out["split"]
    assert env.regions.tobytes() == today["envelopes"].regions.tobytes()
    assert len(aln) == len(split["items"]) == len(out["domain_bits"]) and aln.items.tobytes() == split["items"].tobytes()
    assert split["ensembles"].stats["truncated"] == 0
    for s in two_copy:
        g = [j for j, r in enumerate(env.regions) if r["seq"] == s]
        assert len(g) == 1 and split["multidomain"][g[0]], (s, env.regions)
        mine = np.flatnonzero(split["region"] == g[0])
        assert len(mine) == 2, (s, split["items"][mine])  # two alignment items in place of the region
        a, b = split["items"][mine]
        assert a["seq"] == b["seq"] == s and a["i_from"] < b["i_from"] and a["i_to"] < b["i_to"]
        for it, (first, last), other in zip((a, b), planted, cores[::-1]):
            inside = min(int(it["i_to"]), last) - max(int(it["i_from"]), first) + 1
            assert inside >= 0.8 * (last - first + 1)
            assert int(it["i_to"]) < other[0] or int(it["i_from"]) > other[1]
        assert np.all(split["prob"][mine] >= 0.25) and np.all(split["prob"][mine] <= 1.0)  # the rule's min_posterior
        bits_ = out["domain_bits"][mine]
        assert np.all(np.isfinite(bits_))  # each item has domain_bits of its own
        assert len(aln.domains_of(int(mine[0]))) >= 1
    # the single-copy controls are not split: their items are their regions
    for s in (25, 27):
        g = [j for j, r in enumerate(env.regions) if r["seq"] == s]
        assert len(g) == 1 and not split["multidomain"][g[0]]
        mine = np.flatnonzero(split["region"] == g[0])
        assert len(mine) == 1 and split["prob"][mine[0]] == 1.0
        assert split["items"][mine[0]]["i_from"] == env.regions[g[0]]["i_from"]

    # sample_batch by hand: the defaults are HMMER's, and an item's samples do not depend on the batch
    ens = dom.sample_batch(codes=codes, offsets=offsets, envelopes=env, keep_matrix=True)
    assert ens.n_samples == 200 and ens.seed == 42 and len(ens) == len(env.regions)
    g = [j for j, r in enumerate(env.regions) if r["seq"] == two_copy[0]][0]
    alone = dom.sample_batch(codes=codes, offsets=offsets, items=[tuple(int(env.regions[g][f]) for f in
                                                                        ("seq", "i_from", "i_to"))])
    assert alone.segments_of(0).tobytes() == ens.segments_of(g).tobytes()
    fm, fi, fd, rec = ens.matrix(g)
    r = env.regions[g]
    Lc = int(offsets[int(r["seq"]) + 1] - offsets[int(r["seq"])])
    want = msv.spl_sample(fm, fi, fd, rec, dom.transition_scores, (dom.tr_B_Mk, dom.tr_E_C, dom.tr_E_J), Lc=Lc,
                          seq=int(r["seq"]), i_from=int(r["i_from"]), i_to=int(r["i_to"]), sample=7)
    assert ens.segments_of(g, 7).tobytes() == want[0].tobytes() and not want[3]
    assert len(ens.cluster(g)) == 2
    with pytest.raises(ValueError):
        msv.search_pipeline(*engines, codes=codes, offsets=offsets, dom_engine=dom, split=True)
    dom.close()


def test_cpp_split_regions(tmp_path):
    """tests/cpp/test_split.cpp: the C++ Domain_HMM::split_regions on the pipeline test's two-copy batch gives the
    items of the Python surface exactly (the same library calls with the same defaults)."""
    import subprocess
    hmm_path = os.path.join(ROOT, "data", "profile_HMMs", "100.hmm")
    hmm = msv.Profile_HMM(hmm_path)
    model = forward_lib.tables(hmm)
    (cc, co), _, _ = split_lib.copies_batch(model)
    codes, offsets = cc, co  # the two-copy homolog and its single-copy control: one region each
    fasta = tmp_path / "copies.fsa"
    with open(fasta, "w") as f:
        for s in range(len(offsets) - 1):
            seq = "".join(msv.AMINO_ACIDS[c] for c in codes[int(offsets[s]):int(offsets[s + 1])])
            f.write(f">s{s}\n{seq}\n")
    exe = os.path.join(ROOT, "hmm_fasta_viterbi_amd", "lib", "test_split")
    r = subprocess.run([exe, hmm_path, str(fasta)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "test_split passed" in r.stdout, r.stdout + r.stderr
    got = [tuple(int(x) for x in line.split()[1:4]) + (int(line.split()[5]), float(line.split()[7]))
           for line in r.stdout.splitlines() if line.startswith("item ")]
    dom = msv.Domain_HMM(hmm, device=0)
    env = dom.decode_batch(codes=codes, offsets=offsets)
    split = dom.split_regions(env, codes=codes, offsets=offsets)
    want = [(int(it["seq"]), int(it["i_from"]), int(it["i_to"]), int(g), float(p))
            for it, g, p in zip(split["items"], split["region"], split["prob"])]
    assert list(split["multidomain"]) == [True, False] and len(want) == 3
    assert [g[:4] for g in got] == [w[:4] for w in want], (got, want)
    assert [np.float32(g[4]) for g in got] == [np.float32(w[4]) for w in want]  # (printed with nine digits)
    dom.close()
