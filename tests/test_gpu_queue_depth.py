"""Every kernel variant past one sequence per wave, BITWISE against the oracle.

Every kernel here runs a persistent grid whose launcher starts no more workgroups than the batch needs, so a
batch no larger than the grid's capacity gives each wave (lane group, team) exactly one sequence: the dequeue,
the per-sequence resets, the many-sequence form of the row loop (vit_kernel.hip `few`), the teams' row stamp /
`next` record / skipped-sequence exchange (vit_team.hip) and the MSV streams' refill, junk streams and
fetch-ahead (msv_kernel_body.inc) never run.  The other bitwise tests stay far below those capacities.  Here
every launch asserts n > 2 * capacity (queue_batches.py: a pigeonhole bound, read from describe()), so some
stream scores a third sequence, and the two launches either side of the capacity (n = capacity, capacity + 1)
take both sides of `few` / of the first-index mapping and the first dequeue.

The queue is deep, not long: sequences of length U[1, 130] (the 64-row residue blocks and the two-row loops
need lengths that cross 64 and 128), with profile-emitted sequences and the edge lengths 0..129 throughout the
queue.  Each case prints `QDEPTH <case> capacity=<c> n=<n> seconds=<t>` (pytest -s).
"""
import ctypes as C
import os
import re
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import hmm_fasta_viterbi_amd as msv
from hmm_fasta_viterbi_amd import _native
from hmm_fasta_viterbi_amd.synthetic import concat_batches, homolog_batch, random_batch, write_hmm
from oracle_lib import PROFILES, OracleProfile, bits, oracle, profile_path
from queue_batches import (msv_capacity, msv_groups, msv_streams, prefix, queue_batch, take_sequences,
                           viterbi_capacity)

THREADS = min(16, os.cpu_count() or 1)  # host threads of the oracle
_hmm = {}


def hmm(path):
    if path not in _hmm:
        _hmm[path] = msv.Profile_HMM(profile_path(path) if path in PROFILES else path)
    return _hmm[path]


def report(case, capacity, n, t0):
    print(f"QDEPTH {case} capacity={capacity} n={n} seconds={time.perf_counter() - t0:.2f}")


def same(got, want):
    """Bitwise equality; on failure the first differing indices (located against the capacity by the caller)."""
    g, w = bits(got), bits(want)
    if np.array_equal(g, w):
        return True
    bad = np.nonzero(g != w)[0]
    print(f"{len(bad)} of {len(g)} scores differ, first at {bad[:12].tolist()}: got {np.asarray(got)[bad[:6]]} "
          f"want {np.asarray(want)[bad[:6]]}")
    return False


def tables_scores(msc, tsc, consts, codes, offsets):
    """oracle_lib.vit_score_tables (the oracle's Viterbi DP over caller tables) over THREADS host threads."""
    L = oracle()
    msc = np.ascontiguousarray(msc, np.float32)
    tsc = np.ascontiguousarray(tsc, np.float32)
    codes = np.ascontiguousarray(codes, np.uint8)
    offsets = np.ascontiguousarray(offsets, np.uint64)
    n = len(offsets) - 1
    out = np.zeros(n, np.float32)
    base = codes.ctypes.data if codes.size else None
    cuts = np.linspace(0, n, THREADS + 1).astype(np.int64)

    def run(k):
        lo, hi = int(cuts[k]), int(cuts[k + 1])
        if hi > lo:
            L.oracle_vit_score_tables(msc.ctypes.data, None, tsc.ctypes.data, msc.shape[1],
                                      *[float(x) for x in consts], base, offsets[lo:].ctypes.data, hi - lo,
                                      out[lo:].ctypes.data)

    with ThreadPoolExecutor(THREADS) as ex:
        list(ex.map(run, range(THREADS)))
    return out


# ---------------------------------------------------------------------------------------------------------
# 2. Viterbi: every compiled variant, forced on the largest bundled profile it covers
# ---------------------------------------------------------------------------------------------------------
def vit_shape(name):
    """(states covered, informative insert scores) of a Viterbi variant name."""
    m = re.match(r"vit_(?:w(\d+)_)?s(\d+)_", name)
    return 64 * int(m.group(2)) * int(m.group(1) or 1), name.endswith("i")


def vit_profile_of(name):
    states, _ = vit_shape(name)
    return [p for p in PROFILES if int(p.split(".")[0]) <= states][-1]


def vit_group(name):
    return vit_profile_of(name), 1 if vit_shape(name)[1] else 0


# variants that share a (profile, insert mode) run next to each other: the group's batch and oracle scores are
# made once, at the largest n the group needs, and only the latest group is kept
VIT_VARIANTS = sorted(msv.Viterbi_HMM.variants(), key=lambda v: (int(vit_group(v)[0].split(".")[0]), vit_group(v)[1]))
TEAM_VARIANTS = [v for v in msv.Viterbi_HMM.variants() if v.startswith("vit_w")]
_vit_latest = {}


def forced(name):
    prof, isc = vit_group(name)
    e = msv.Viterbi_HMM(hmm(prof), insert_mode=isc)
    e.set_variant(name)
    assert e.describe()["variant"] == name
    return e


def vit_group_batch(group):
    if _vit_latest.get("group") != group:
        _vit_latest.clear()
        prof, isc = group
        caps = {}
        for v in VIT_VARIANTS:
            if vit_group(v) == group:
                e = forced(v)
                caps[v] = viterbi_capacity(e.describe())
                e.close()
        n = 3 * max(caps.values()) + 17
        codes, offsets = queue_batch(hmm(prof).match_emissions, 1000 + int(prof.split(".")[0]) + isc, n)
        want = OracleProfile(prof).vit_score_batch(codes, offsets, isc, threads=THREADS)
        _vit_latest.update(group=group, caps=caps, codes=codes, offsets=offsets, want=want)
    return _vit_latest


@pytest.mark.parametrize("name", VIT_VARIANTS)
def test_viterbi_every_variant_three_rounds_deep(name):
    """Each Viterbi instantiation on 3 * capacity + 17 sequences (some wave or team scores a third one: the
    dequeue, the per-sequence resets, the plain lazy-F form that `few` hides, the teams' records across
    sequences), and on exactly capacity / capacity + 1 (both sides of `few` and of the first dequeue)."""
    t0 = time.perf_counter()
    g = vit_group_batch(vit_group(name))
    e = forced(name)
    capacity = viterbi_capacity(e.describe())
    assert capacity == g["caps"][name]
    n = 3 * capacity + 17
    assert n > 2 * capacity and n <= len(g["want"])
    for m in (n, capacity, capacity + 1):
        codes, offsets = prefix(g["codes"], g["offsets"], m)
        got = e.score_batch(codes=codes, offsets=offsets)
        assert same(got, g["want"][:m]), (name, vit_group(name), m, capacity)
    e.close()
    report(f"viterbi {name} {vit_group(name)[0]}", capacity, n, t0)


# ---------------------------------------------------------------------------------------------------------
# 3. Team exchange at depth: the stress tables, and the bench picks on long sequences in a row
# ---------------------------------------------------------------------------------------------------------
class CustomVit:
    """A Viterbi profile over caller tables (msv_vit_profile_create) with one variant forced."""

    def __init__(self, msc, tsc, consts, model_length, name):
        self.L = _native.lib()
        self.p = C.c_void_p()
        tsc = np.ascontiguousarray(tsc, np.float32)
        assert self.L.msv_vit_profile_create(0, msc.ctypes.data, None, tsc.ctypes.data, model_length, *consts,
                                             C.byref(self.p)) == 0
        assert self.L.msv_vit_profile_set_variant(self.p, name.encode()) == 0

    def describe(self):
        info = _native.VitInfo()
        assert self.L.msv_vit_profile_describe(self.p, C.byref(info)) == 0
        return info.as_dict()

    def score(self, codes, offsets):
        out = np.zeros(len(offsets) - 1, np.float32)
        assert self.L.msv_vit_score_batch(self.p, codes.ctypes.data if codes.size else None, offsets.ctypes.data,
                                          len(offsets) - 1, out.ctypes.data, None) == 0
        return out

    def close(self):
        if self.p:
            self.L.msv_vit_profile_destroy(self.p)
            self.p = None


@pytest.mark.parametrize("name", TEAM_VARIANTS)
def test_team_exchange_three_rounds_deep(name):
    """vit_team.hip's state that outlives a sequence -- the row stamp and its parity, the sequence ordinal and
    the `next` record, the late take() with its one-row fallback, the extra exchange of a skipped (empty)
    sequence and the extra stamp of the C exchange -- with 3 * capacity + 17 sequences per launch on the two
    tables that stress the exchange: D -> D at 0.995 (D chains cross the waves' boundary every row) and
    tr_E_C != tr_E_J (per-lane C partials reduced across the team, one more stamp per sequence)."""
    t0 = time.perf_counter()
    prof = vit_profile_of(name)
    o = OracleProfile(prof)
    _, tsc0 = o.vit_tables(0)
    msc = o.emission_scores()
    b, c, j = o.constants()
    stress = tsc0.copy()
    stress[:, 6] = np.float32(np.log(np.float32(0.995)))
    stress[:, 2] = np.float32(np.log(np.float32(0.3)))
    stress[:, 5] = np.float32(np.log(np.float32(0.9)))
    batch = None
    for what, tsc, consts in (("D->D 0.995", stress, (b, c, j)),
                              ("tr_E_C != tr_E_J", tsc0, (b, float(np.float32(c) - np.float32(0.75)), j))):
        e = CustomVit(msc, tsc, consts, o.model_length, name)
        try:
            info = e.describe()
            assert info["variant"] == name and info["waves_per_sequence"] >= 1
            capacity = viterbi_capacity(info)
            n = 3 * capacity + 17
            assert n > 2 * capacity
            if batch is None:
                batch = queue_batch(hmm(prof).match_emissions, 2000 + int(prof.split(".")[0]), n)
            codes, offsets = batch
            assert len(offsets) - 1 == n
            want = tables_scores(msc, tsc, consts, codes, offsets)
            assert same(e.score(codes, offsets), want), (name, prof, what, capacity)
        finally:
            e.close()
    report(f"team {name} {prof} (2 tables)", capacity, n, t0)


@pytest.mark.parametrize("name,prof", [("vit_w1_s22_ea", "1400.hmm"), ("vit_w2_s19_gb", "2405.hmm")])
def test_team_bench_picks_long_sequences_in_a_row(name, prof):
    """The two bench picks on cfg3's survivor lengths, two rounds deep (2 * capacity + 5 sequences of length
    U[300, 500], a quarter of them emitted by the profile), with 48 sequences of cfg5's lengths (U[1500, 2500])
    scattered among them: a team scores long sequences in a row, thousands of row stamps apart."""
    t0 = time.perf_counter()
    e = msv.Viterbi_HMM(hmm(prof))
    e.set_variant(name)
    info = e.describe()
    assert info["variant"] == name
    capacity = viterbi_capacity(info)
    m = 2 * capacity + 5
    seed = 3000 + int(prof.split(".")[0])
    codes, offsets = concat_batches(random_batch(seed, m - m // 4, 300, 500),
                                    homolog_batch(hmm(prof).match_emissions, seed + 1, m // 4, 300, 500),
                                    random_batch(seed + 2, 48, 1500, 2500))
    n = m + 48
    codes, offsets = take_sequences(codes, offsets, np.random.Generator(np.random.PCG64(seed + 3)).permutation(n))
    assert len(offsets) - 1 == n and n > 2 * capacity
    want = OracleProfile(prof).vit_score_batch(codes, offsets, threads=THREADS)
    assert same(e.score_batch(codes=codes, offsets=offsets), want), (name, prof, capacity)
    e.close()
    report(f"team-long {name} {prof}", capacity, n, t0)


# ---------------------------------------------------------------------------------------------------------
# 4./5. the picks: a single-wave short-row pick, the W = 1 team, a W = 2 team
# ---------------------------------------------------------------------------------------------------------
PICKS = ["100.hmm", "1400.hmm", "2405.hmm"]
_pick = {}


def pick(prof):
    """The automatic variant of a pick with its batch of 3 * capacity + 17 and the oracle's scores."""
    if prof not in _pick:
        e = msv.Viterbi_HMM(hmm(prof))
        info = e.describe()
        capacity = viterbi_capacity(info)
        n = 3 * capacity + 17
        codes, offsets = queue_batch(hmm(prof).match_emissions, 4000 + int(prof.split(".")[0]), n)
        want = OracleProfile(prof).vit_score_batch(codes, offsets, threads=THREADS)
        _pick[prof] = dict(e=e, info=info, capacity=capacity, n=n, codes=codes, offsets=offsets, want=want)
    return _pick[prof]


def test_the_picks_are_the_three_kinds():
    w = {p: pick(p)["info"] for p in PICKS}
    assert w["100.hmm"]["waves_per_sequence"] == 1 and not w["100.hmm"]["variant"].startswith("vit_w")
    assert w["100.hmm"]["states_per_lane"] <= 4  # the short-row hops form exists for S <= 4
    assert w["1400.hmm"]["variant"].startswith("vit_w1_") and w["1400.hmm"]["waves_per_sequence"] == 1
    assert w["2405.hmm"]["variant"].startswith("vit_w2_") and w["2405.hmm"]["waves_per_sequence"] == 2


def replace_sequences(codes, offsets, plants):
    """The batch with sequence i replaced by plants[i] (uint8 codes) for every key i."""
    pieces, lens = [], np.diff(offsets.astype(np.int64))
    at = 0
    for i in sorted(plants):
        pieces.append(codes[int(offsets[at]):int(offsets[i])])
        pieces.append(np.asarray(plants[i], np.uint8))
        lens[i] = len(plants[i])
        at = i + 1
    pieces.append(codes[int(offsets[at]):int(offsets[-1])])
    out = np.zeros(len(lens) + 1, np.uint64)
    np.cumsum(lens, out=out[1:])
    return np.concatenate(pieces), out


def device_launch(e, codes, offsets, stream, fill=7.0):
    """One msv_vit_score_batch_device launch of a host batch on `stream`; returns (scores tensor, keep-alive)."""
    import torch
    dev = torch.device("cuda:0")
    n = len(offsets) - 1
    d_res = torch.from_numpy(np.ascontiguousarray(codes)).to(dev)
    d_off = torch.from_numpy(np.ascontiguousarray(offsets).view(np.int64)).to(dev)
    d_sc = torch.full((n,), fill, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    e.score_batch_device(d_res.data_ptr(), codes.size, d_off.data_ptr(), n, d_sc.data_ptr(), None, None,
                         stream.cuda_stream)
    return d_sc, (d_res, d_off)


@pytest.mark.parametrize("prof", PICKS)
def test_errors_do_not_leak_along_a_queue(prof):
    """Six sequences holding a residue code >= 20 (three among the statically assigned indices, three in the
    queue), two sequences one residue past the reserved length, an empty sequence straight after each, in a
    launch three rounds deep: +inf / NaN / -inf exactly there, every other score bitwise -- the wave that met the
    error scores its next sequences clean (`maxcode`, the residue prefetch, the teams' skipped-sequence
    exchange) -- check() reports once, and a clean launch of the rest follows bitwise."""
    import torch
    t0 = time.perf_counter()
    g = pick(prof)
    e, capacity, n, want = g["e"], g["capacity"], g["n"], g["want"]
    too_long = e.describe()["max_length"] + 1  # (not reserved: the launch must refuse it)
    rng = np.random.Generator(np.random.PCG64(11))
    bad_at = [5, capacity // 2, capacity - 2, capacity, 2 * capacity + 3, n - 2]
    long_at = [capacity // 3, capacity + capacity // 2]
    plants = {}
    # (length, position of the bad code, the code): one residue only; past a 64-row block; the last residue
    for i, (length, pos, code) in zip(bad_at, [(1, 0, 20), (66, 65, 21), (130, 129, 255), (129, 0, 20), (64, 63, 37),
                                               (2, 1, 128)]):
        s = rng.integers(0, 20, length, dtype=np.uint8)
        s[pos] = code
        plants[i] = s
    for i in long_at:
        plants[i] = rng.integers(0, 20, too_long, dtype=np.uint8)
    planted = sorted(plants)
    for i in planted:
        plants[i + 1] = np.zeros(0, np.uint8)
    assert len(plants) == 16 and max(plants) == n - 1
    assert sum(i < capacity for i in bad_at) == 3 and sum(i >= capacity for i in bad_at) == 3
    codes, offsets = replace_sequences(g["codes"], g["offsets"], plants)
    assert len(offsets) - 1 == n and n > 2 * capacity
    st = torch.cuda.Stream(torch.device("cuda:0"))
    d_sc, keep = device_launch(e, codes, offsets, st)
    st.synchronize()
    with pytest.raises(IndexError):  # (a bad residue outranks a too-long sequence)
        e.check(st.cuda_stream)
    e.check(st.cuda_stream)  # reported once, then clean
    got = d_sc.cpu().numpy()
    assert np.all(np.isposinf(got[bad_at])), got[bad_at]
    assert np.all(np.isnan(got[long_at])), got[long_at]
    assert np.all(np.isneginf(got[[i + 1 for i in planted]]))
    rest = np.ones(n, bool)
    rest[sorted(plants)] = False
    assert same(got[rest], want[rest]), (prof, capacity)
    # the same batch without the planted sequences
    c2, o2 = take_sequences(g["codes"], g["offsets"], np.nonzero(rest)[0])
    d_sc2, keep2 = device_launch(e, c2, o2, st)
    st.synchronize()
    e.check(st.cuda_stream)
    assert same(d_sc2.cpu().numpy(), want[rest]), (prof, capacity)
    report(f"errors {g['info']['variant']} {prof}", capacity, n, t0)


@pytest.mark.parametrize("prof", ["100.hmm", "2405.hmm"])
def test_three_launches_back_to_back_deeper_than_the_grid(prof):
    """Three launches queued on one stream with no synchronisation between them, of 3 * capacity + 17, 5 and
    2 * capacity + 1 sequences: each bitwise.  A launch's counter slot resets itself (its last wave), here after
    queues that really advanced."""
    import torch
    t0 = time.perf_counter()
    g = pick(prof)
    e, capacity, n = g["e"], g["capacity"], g["n"]
    assert n > 2 * capacity
    st = torch.cuda.Stream(torch.device("cuda:0"))
    dev = torch.device("cuda:0")
    d_res = torch.from_numpy(g["codes"]).to(dev)
    d_off = torch.from_numpy(g["offsets"].view(np.int64)).to(dev)
    sizes = (n, 5, 2 * capacity + 1)
    outs = [torch.full((m,), 7.0, dtype=torch.float32, device=dev) for m in sizes]
    torch.cuda.synchronize()
    for m, d_sc in zip(sizes, outs):  # (a prefix of a CSR batch is a batch: the same arrays, n = m)
        e.score_batch_device(d_res.data_ptr(), int(g["offsets"][m]), d_off.data_ptr(), m, d_sc.data_ptr(), None, None,
                             st.cuda_stream)
    st.synchronize()
    e.check(st.cuda_stream)
    for m, d_sc in zip(sizes, outs):
        assert same(d_sc.cpu().numpy(), g["want"][:m]), (prof, m, capacity)
    report(f"back-to-back {g['info']['variant']} {prof}", capacity, n, t0)


# ---------------------------------------------------------------------------------------------------------
# 5. survivor lists deeper than the grid
# ---------------------------------------------------------------------------------------------------------
_msv_engine = {}


def msv_engine(prof):
    if prof not in _msv_engine:
        _msv_engine[prof] = msv.MSV_HMM(hmm(prof))
    return _msv_engine[prof]


@pytest.mark.parametrize("prof", ["400.hmm", "2405.hmm"])
def test_filter_pipeline_every_sequence_survives(prof):
    """filter_pipeline with F1 = 1: every sequence survives (P <= 1, the empty ones included), so the Viterbi
    launch takes a device survivors list of n > 2 * capacity entries, longest first; MSV and Viterbi scores
    bitwise, every sequence passed."""
    t0 = time.perf_counter()
    m = msv_engine(prof)
    e = msv.Viterbi_HMM(hmm(prof))
    capacity = viterbi_capacity(e.describe())
    n = 3 * capacity + 17
    assert n > 2 * capacity
    codes, offsets = queue_batch(hmm(prof).match_emissions, 5000 + int(prof.split(".")[0]), n)
    o = OracleProfile(prof)
    want_m = o.score_batch(codes, offsets, threads=THREADS)
    want_v = o.vit_score_batch(codes, offsets, threads=THREADS)
    assert np.all(m.pvalues(want_m, offsets) <= 1.0)
    msc, passed, vsc, vpv = msv.filter_pipeline(m, e, codes=codes, offsets=offsets, F1=1.0)
    assert same(msc, want_m), prof
    assert passed.all() and len(passed) == n
    assert same(vsc, want_v), (prof, capacity)
    e.close()
    report(f"filter F1=1 {prof}", capacity, n, t0)


@pytest.mark.parametrize("prof", ["400.hmm", "2405.hmm"])
def test_filter_pipeline_survivors_beyond_the_grid(prof):
    """filter_pipeline at hmmsearch's F1 = 0.02 on a batch heavy in profile-emitted sequences: the survivors
    (asserted on the oracle's side) outnumber the Viterbi grid's capacity and are fewer than half the batch, so
    the launch is sized for n, its list is a count in device memory, and the grid queues through it."""
    t0 = time.perf_counter()
    m = msv_engine(prof)
    e = msv.Viterbi_HMM(hmm(prof))
    capacity = viterbi_capacity(e.describe())
    # ~0.9 of the emitted sequences of length 60..130 and ~0.02-0.06 of the random ones pass the MSV filter
    n_hom, n_rand = capacity + capacity // 3, 3 * capacity
    n = n_hom + n_rand
    seed = 6000 + int(prof.split(".")[0])
    codes, offsets = concat_batches(homolog_batch(hmm(prof).match_emissions, seed, n_hom, 60, 130),
                                    random_batch(seed + 1, n_rand, 0, 130))
    codes, offsets = take_sequences(codes, offsets, np.random.Generator(np.random.PCG64(seed + 2)).permutation(n))
    o = OracleProfile(prof)
    want_m = o.score_batch(codes, offsets, threads=THREADS)
    want_pass = m.pvalues(want_m, offsets) <= 0.02
    survivors = int(want_pass.sum())
    assert capacity < survivors < n / 2, (capacity, survivors, n)
    want_v = o.vit_score_batch(codes, offsets, threads=THREADS)
    msc, passed, vsc, vpv = msv.filter_pipeline(m, e, codes=codes, offsets=offsets, F1=0.02)
    assert same(msc, want_m), prof
    assert np.array_equal(passed, want_pass)
    assert same(vsc[passed], want_v[passed]), (prof, capacity, survivors)
    assert np.all(np.isneginf(vsc[~passed]))
    e.close()
    report(f"filter F1=0.02 {prof} survivors={survivors}", capacity, n, t0)


# ---------------------------------------------------------------------------------------------------------
# 6. MSV: every compiled variant at depth
# ---------------------------------------------------------------------------------------------------------
SYNTHETIC = (2600, 3000, 3500, 4096)  # model lengths past the bundled profiles' 2405 (seeded HMMER3 files)


def msv_shape(name):
    parts = name.split("_")
    return int(parts[1][1:]), int(parts[2][1:])


def msv_assignment():
    """Every non-exp MSV variant on the largest model it covers, as test_every_variant_matches_oracle assigns
    them: {profile (a bundled name or a synthetic length): [variants]}.  A variant smaller than the smallest
    bundled profile (16 x 4 states; that test leaves it out) gets a synthetic model of exactly its states."""
    lengs = {p: msv.Profile_HMM(profile_path(p)).model_length - 1 for p in PROFILES}
    lengs.update({leng: leng for leng in SYNTHETIC})
    by_prof = {}
    for name in msv.MSV_HMM.variants():
        if name.startswith("exp"):
            continue
        g, s = msv_shape(name)
        fits = [p for p in lengs if lengs[p] <= g * s]
        if not fits:
            lengs[g * s] = g * s
            fits = [g * s]
        by_prof.setdefault(max(fits, key=lambda p: lengs[p]), []).append(name)
    return by_prof, lengs


MSV_BY_PROF, MSV_LENG = msv_assignment()
MSV_CELLS = 4e9  # oracle cells per case: a few seconds of the host's time


def msv_profile_path(prof, tmp_path):
    if prof in PROFILES:
        return profile_path(prof)
    path = str(tmp_path / f"syn{prof}.hmm")
    write_hmm(path, prof, prof)
    return path


def device_msv(e, codes, offsets, st):
    import torch
    dev = torch.device("cuda:0")
    n = len(offsets) - 1
    d_res = torch.from_numpy(np.ascontiguousarray(codes)).to(dev)
    d_off = torch.from_numpy(np.ascontiguousarray(offsets).view(np.int64)).to(dev)
    d_sc = torch.full((n,), 7.0, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    e.score_batch_device(d_res.data_ptr(), codes.size, d_off.data_ptr(), n, d_sc.data_ptr(), None, st.cuda_stream)
    st.synchronize()
    e.check(st.cuda_stream)
    return d_sc.cpu().numpy()


def test_msv_assignment_covers_every_variant():
    names = [v for v in msv.MSV_HMM.variants() if not v.startswith("exp")]
    assert sorted(sum(MSV_BY_PROF.values(), [])) == sorted(names) and len(names) >= 40


@pytest.mark.parametrize("prof", sorted(MSV_BY_PROF, key=lambda p: MSV_LENG[p]), ids=str)
def test_msv_every_variant_three_rounds_deep(prof, tmp_path):
    """Each MSV instantiation forced on 3 * capacity + 17 sequences in ONE device launch in queue order (no
    longest-first order: empty sequences -- junk streams -- and 1-residue ones sit in mid-queue), so a lane
    group's streams refill (begin, `pending`), fetch ahead and, for S >= 64, the young waves retire with the
    queue still running; then through the host call (score_batch: longest first, in pieces past 4 MiB)."""
    import torch
    t0 = time.perf_counter()
    path = msv_profile_path(prof, tmp_path)
    names = MSV_BY_PROF[prof]
    e = msv.MSV_HMM(hmm(path))
    caps = {}
    for name in names:
        e.set_variant(name)
        info = e.describe()
        assert info["variant"] == name
        caps[name] = msv_capacity(info, name)
    n_max = 3 * max(caps.values()) + 17
    # the queue has to be deep, not long: shorter sequences where the oracle would take too long
    lmax = int(min(130, max(40, 2 * MSV_CELLS / (n_max * MSV_LENG[prof]))))
    codes, offsets = queue_batch(hmm(path).match_emissions, 7000 + MSV_LENG[prof], n_max, lmax=lmax)
    want = OracleProfile(path).score_batch(codes, offsets, threads=THREADS)
    st = torch.cuda.Stream(torch.device("cuda:0"))
    for name in names:
        e.set_variant(name)
        n = 3 * caps[name] + 17
        assert n > 2 * caps[name] and n <= n_max
        c, o = prefix(codes, offsets, n)
        assert same(device_msv(e, c, o, st), want[:n]), (prof, name, caps[name], "device launch")
        assert same(e.score_batch(codes=c, offsets=o), want[:n]), (prof, name, caps[name], "host call")
        print(f"QDEPTH msv {name} {prof} capacity={caps[name]} n={n} lmax={lmax}")
    e.close()
    report(f"msv {prof} ({len(names)} variants)", max(caps.values()), n_max, t0)


@pytest.mark.parametrize("G", [4, 8, 16, 32, 64])
def test_msv_first_index_mappings(G):
    """n = n_groups and n = n_groups + 1 in one launch each, for one single-stream variant of each group width:
    the two mappings of a lane group to its first index (dealt in rounds over the SIMDs / block by block), the
    second one with exactly one sequence left to the counter."""
    import torch
    t0 = time.perf_counter()
    prof, name = next((p, v) for p in sorted((p for p in MSV_BY_PROF if p in PROFILES), key=lambda p: MSV_LENG[p])
                      for v in MSV_BY_PROF[p] if msv_shape(v)[0] == G and msv_streams(v) == 1)
    e = msv.MSV_HMM(hmm(prof))
    e.set_variant(name)
    info = e.describe()
    assert info["variant"] == name and info["lanes_per_group"] == G
    groups = msv_groups(info)
    assert groups == msv_capacity(info, name)
    codes, offsets = queue_batch(hmm(prof).match_emissions, 8000 + G, groups + 1)
    want = OracleProfile(prof).score_batch(codes, offsets, threads=THREADS)
    st = torch.cuda.Stream(torch.device("cuda:0"))
    for n in (groups, groups + 1):
        c, o = prefix(codes, offsets, n)
        assert same(device_msv(e, c, o, st), want[:n]), (prof, name, groups, n)
    e.close()
    report(f"msv-first-index {name} {prof}", groups, groups + 1, t0)
