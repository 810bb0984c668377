"""Every kernel variant at the edges of its capacity, BITWISE against the oracle.

The other bitwise tests force each variant on the largest bundled profile it covers, so the top states of the last
lane (wave, team member) are -inf padding in every run, and their batches (uniform sequences, homolog_batch cores
from a uniform random start) never put a best path through the last states of a large model
(test_state_batches.py).  Here every variant is forced on seeded synthetic models of exactly its capacity C
(G * S states for MSV, 64 * S * W for Viterbi), of C - S + 1 (one real state in the last lane) and C - S (the
last lane all padding), teams also at 64 * S and 64 * S + 1 (the second wave all padding / one state); the
automatic choice runs at every capacity C and C + 1, where an off-by-one in a picker's comparison would select a
plan one state too small; and tables with a column knocked out (-inf inside the model) run against the CPU DPs.

The batches (state_batches.boundary_batch) are aimed: tail homologs whose core ends in state LENG, window
homologs across lane boundaries of the variant's layout (read from the table builders: install_plan,
install_coop_table in msv_device.cpp, install in vit_device.cpp), gapped paths into the last nodes for
Viterbi, the edge lengths 0, 1, 2, 63, 64, 65, and uniform sequences between them in the queue."""
import ctypes as C
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import hmm_fasta_viterbi_amd as msv
from hmm_fasta_viterbi_amd import _native
from hmm_fasta_viterbi_amd.synthetic import concat_batches, random_batch, write_hmm
from oracle_lib import OracleProfile, bits, vit_score_tables
from state_batches import boundary_batch, knock_out, numpy_msv, tail_homolog_batch, window_homolog_batch

MAX_STATES = 4096  # the largest model the compiled family covers (test_gpu_model_lengths.py)

# The cooperative variants (msv_coop_variants.inc): name -> (waves, S, halo, SA); states() = waves * (64 S - halo).
# Pinned here: the tests below observe each capacity as the change of describe()'s coop_variant across it.
COOP = {
    "msv_coop_w4_s2": (4, 2, 16, 2),
    "msv_coop_w4_s4": (4, 4, 16, 4),
    "msv_coop_w4_s6": (4, 6, 18, 6),
    "msv_coop_w4_s8_a6": (4, 8, 16, 6),
    "msv_coop_w4_s10_a6": (4, 10, 20, 6),
}


def coop_states(name):
    w, s, halo, _ = COOP[name]
    return w * (64 * s - halo)


COOP_STATES = {name: coop_states(name) for name in COOP}  # 448, 960, 1464, 1984, 2480


def msv_layout(name):
    """(G, S, SA) of an MSV variant name msv_g<G>_s<S>[_a<SA>]_w..: lane gl holds states gl S + 1 .. gl S + S, a
    split variant its first SA of them in LDS and the rest in the L2 table."""
    m = re.match(r"msv_g(\d+)_s(\d+)(?:_a(\d+))?_w", name)
    return int(m.group(1)), int(m.group(2)), int(m.group(3) or 0)


def vit_layout(name):
    """(S, W, informative insert scores) of a Viterbi variant name: virtual lane l of the team's 64 W holds states
    l S + 1 .. l S + S."""
    m = re.match(r"vit_(?:w(\d+)_)?s(\d+)_", name)
    return int(m.group(2)), int(m.group(1) or 1), name.endswith("i")


def msv_boundaries(name):
    """State boundaries b | b + 1 of the variant's layout worth a window: between lanes 0|1, 15|16 (DPP rows),
    31|32 (the wave's halves), G/2 - 1 | G/2 and the last two lanes; for split variants between the LDS and L2
    parts of the first, a middle and the last lane."""
    g, s, sa = msv_layout(name)
    out = {lane * s for lane in (1, 16, 32, g // 2, g - 1) if 1 <= lane < g}
    if sa:
        out |= {lane * s + sa for lane in (0, g // 2, g - 1)}
    return sorted(out)


def vit_boundaries(name):
    """Lane boundaries 0|1, 15|16, 31|32, 62|63 of each wave of the team, the wave boundary 63|64, and the last
    lane of the team."""
    s, w, _ = vit_layout(name)
    return sorted({(64 * k + lane) * s for k in range(w) for lane in (1, 16, 32, 63, 64) if 64 * k + lane < 64 * w})


def coop_boundaries(name):
    """The cooperative layout (install_coop_table): wave w's own states start at w (64 S - halo) + 1 and its halo
    lanes repeat the halo states below; windows across each wave boundary, each halo's first state, a lane
    boundary inside a wave and, split, the LDS | L2 boundary of a lane in the first and the last wave."""
    w, s, halo, sa = COOP[name]
    own = 64 * s - halo
    out = {k * own for k in range(1, w)} | {k * own - halo for k in range(1, w)} | {s, own + 7 * s}
    if sa < s:
        out |= {sa, (w - 1) * own - halo + 40 * s + sa}
    return sorted(b for b in out if b >= 1)


MSV_NAMES = [v for v in msv.MSV_HMM.variants() if not v.startswith("exp")]
VIT_NAMES = [v for v in msv.Viterbi_HMM.variants() if not v.startswith("exp")]


def msv_lengths(name):
    g, s, _ = msv_layout(name)
    return [x for x in (g * s, g * s - s + 1, g * s - s) if x >= 1]


def vit_lengths(name):
    s, w, _ = vit_layout(name)
    c = 64 * s * w
    return [x for x in dict.fromkeys((c, c - s + 1, c - s) + ((64 * s, 64 * s + 1) if w == 2 else ())) if x >= 1]


MSV_CAPACITIES = sorted({msv_lengths(n)[0] for n in MSV_NAMES})
VIT_CAPACITIES = {isc: sorted({vit_lengths(n)[0] for n in VIT_NAMES if vit_layout(n)[2] == isc}) for isc in (False, True)}
AUTO_CAPACITIES = sorted(set(MSV_CAPACITIES) | set(VIT_CAPACITIES[False]) | set(VIT_CAPACITIES[True])
                         | set(COOP_STATES.values()))

_models = {}
_wants = {}


def model(leng, tmp_path_factory):
    """(path, parsed profile, oracle profile) of the seeded synthetic model of LENG `leng`, made once per run."""
    if leng not in _models:
        path = str(tmp_path_factory.mktemp("boundaries") / f"syn{leng}.hmm")
        write_hmm(path, leng, 9000 + leng)
        _models[leng] = (path, msv.Profile_HMM(path), OracleProfile(path))
        assert _models[leng][1].model_length == leng + 1
    return _models[leng]


def aimed(leng, boundaries, tmp_path_factory, viterbi=False, insert_mode=0):
    """The boundary batch of the model and its oracle scores, shared by the variants with the same layout."""
    key = (leng, tuple(boundaries), viterbi, insert_mode)
    if key not in _wants:
        _, h, o = model(leng, tmp_path_factory)
        (codes, offsets), where = boundary_batch(h.match_emissions, 100 + leng, boundaries, viterbi=viterbi)
        want = o.vit_score_batch(codes, offsets, insert_mode) if viterbi else o.score_batch(codes, offsets)
        _wants[key] = (codes, offsets, where, want)
    return _wants[key]


def same(got, want, what):
    g, w = bits(got), bits(want)
    if np.array_equal(g, w):
        return True
    bad = np.nonzero(g != w)[0]
    print(f"{what}: {len(bad)} of {len(g)} scores differ, first at {bad[:12].tolist()}: got "
          f"{np.asarray(got)[bad[:6]]} want {np.asarray(want)[bad[:6]]}")
    return False


def device_scores(e, codes, offsets, longest_first=False):
    """One device launch in queue order (d_order NULL: neighbours in the batch share a wave) or longest first."""
    import torch
    dev = torch.device("cuda:0")
    n = len(offsets) - 1
    st = torch.cuda.Stream(dev)
    d_res = torch.from_numpy(np.ascontiguousarray(codes)).to(dev)
    d_off = torch.from_numpy(np.ascontiguousarray(offsets).view(np.int64)).to(dev)
    d_sc = torch.full((n,), 7.0, dtype=torch.float32, device=dev)
    order = None
    if longest_first:
        order = torch.empty(n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    if order is not None:
        e.order_longest_first(d_off.data_ptr(), n, order.data_ptr(), st.cuda_stream)
    e.score_batch_device(d_res.data_ptr(), codes.size, d_off.data_ptr(), n, d_sc.data_ptr(),
                         order.data_ptr() if order is not None else None, st.cuda_stream)
    st.synchronize()
    e.check(st.cuda_stream)
    return d_sc.cpu().numpy()


# ---------------------------------------------------------------------------------------------------------
# 1. every variant forced at its capacity edges
# ---------------------------------------------------------------------------------------------------------
def test_parametrization_covers_every_variant():
    """Every compiled MSV and Viterbi variant is a case below, the pinned cooperative table is the compiled one
    (its names are the only cooperative names any profile reports: test_auto_choice_at_capacity_edges), and every
    cooperative capacity is an automatic-choice case."""
    assert sorted(MSV_NAMES) == sorted(v for v in msv.MSV_HMM.variants() if not v.startswith("exp"))
    assert len(MSV_NAMES) >= 40
    assert sorted(VIT_NAMES) == sorted(msv.Viterbi_HMM.variants()) and len(VIT_NAMES) >= 30
    assert all(msv_lengths(n)[0] in AUTO_CAPACITIES for n in MSV_NAMES)
    assert all(vit_lengths(n)[0] in AUTO_CAPACITIES for n in VIT_NAMES)
    assert [COOP_STATES[n] for n in COOP] == [448, 960, 1464, 1984, 2480]
    assert all(c in AUTO_CAPACITIES for c in COOP_STATES.values())
    assert max(AUTO_CAPACITIES) == MAX_STATES


@pytest.mark.parametrize("name", MSV_NAMES)
def test_msv_variant_at_capacity_edges(name, tmp_path_factory):
    """The variant forced on LENG = C (exact fit), C - S + 1 (one real state in the last lane) and C - S (the last
    lane all padding): one device launch in queue order and the host call (longest first)."""
    g, s, _ = msv_layout(name)
    for leng in msv_lengths(name):
        _, h, _ = model(leng, tmp_path_factory)
        codes, offsets, where, want = aimed(leng, msv_boundaries(name), tmp_path_factory)
        e = msv.MSV_HMM(h)
        try:
            e.set_variant(name)
            info = e.describe()
            assert info["variant"] == name and info["lanes_per_group"] * info["states_per_lane"] == g * s >= leng
            assert e.variant_for(1) == e.variant_for(len(offsets) - 1) == name
            assert same(device_scores(e, codes, offsets), want, f"{name} LENG {leng} device"), (name, leng, where)
            assert same(e.score_batch(codes=codes, offsets=offsets), want, f"{name} LENG {leng} host"), (name, leng)
        finally:
            e.close()


@pytest.mark.parametrize("name", VIT_NAMES)
def test_viterbi_variant_at_capacity_edges(name, tmp_path_factory):
    """The Viterbi variant forced on LENG = C, C - S + 1 and C - S, teams of two waves also on 64 S (the second
    wave all padding) and 64 S + 1 (one state in it); variants with informative insert scores in insert mode 1."""
    s, w, isc = vit_layout(name)
    mode = 1 if isc else 0
    for leng in vit_lengths(name):
        _, h, _ = model(leng, tmp_path_factory)
        codes, offsets, where, want = aimed(leng, vit_boundaries(name), tmp_path_factory, True, mode)
        e = msv.Viterbi_HMM(h, insert_mode=mode)
        try:
            e.set_variant(name)
            info = e.describe()
            assert info["variant"] == name and info["states_per_lane"] == s and info["waves_per_sequence"] == w
            assert same(e.score_batch(codes=codes, offsets=offsets), want, f"{name} LENG {leng}"), (name, leng, where)
        finally:
            e.close()


# ---------------------------------------------------------------------------------------------------------
# 2. the automatic choice at every capacity C and C + 1
# ---------------------------------------------------------------------------------------------------------
def covering_coop(leng):
    """The pinned cooperative variant that must serve a model of LENG `leng`: the smallest covering one."""
    fits = [n for n in COOP if COOP_STATES[n] >= leng]
    return min(fits, key=COOP_STATES.get) if fits else ""


def assert_msv_plans_cover(e, leng, sizes):
    info = e.describe()
    for key in ("variant", "latency_variant", "mid_variant"):
        if info[key]:
            g, s, _ = msv_layout(info[key])
            assert g * s >= leng, (leng, key, info[key])
    assert info["lanes_per_group"] * info["states_per_lane"] >= leng and info["model_length"] == leng + 1
    # the cooperative plan: the pinned variant for this length (so its name changes exactly across each states())
    assert info["coop_variant"] == covering_coop(leng), (leng, info["coop_variant"])
    for n in sizes:
        name = e.variant_for(n)
        if name in COOP:
            assert COOP_STATES[name] >= leng and n <= info["coop_max_n"], (leng, n, name)
        else:
            g, s, _ = msv_layout(name)
            assert g * s >= leng, (leng, n, name)
    return info


@pytest.mark.parametrize("cap", AUTO_CAPACITIES)
def test_auto_choice_at_capacity_edges(cap, tmp_path_factory):
    """Models of LENG = C and C + 1 for every capacity C of the MSV, cooperative and Viterbi families under the
    automatic choice, at one sequence, about 300 and about 6,000 (the sizes that reach the cooperative, latency,
    mid and throughput plans, test_tiny_models_every_plan), tail and window homologs included: bitwise, and every
    plan describe() / variant_for(n) reports covers the model.  Viterbi runs where C is a Viterbi capacity."""
    for leng in (cap, cap + 1):
        if leng > MAX_STATES:
            continue
        _, h, o = model(leng, tmp_path_factory)
        coop = covering_coop(leng)
        bounds = coop_boundaries(coop) if coop else [leng // 2]
        codes, offsets, where, want = aimed(leng, bounds, tmp_path_factory)
        e = msv.MSV_HMM(h)
        try:
            n_small = len(offsets) - 1
            # ~300 and ~6,000: the aimed batch first, then uniform sequences short enough for the oracle
            lmax = int(min(130, max(24, 1.5e9 / (6000 * leng))))
            batches = {1: (codes[int(offsets[where["tail"][0]]):int(offsets[where["tail"][0] + 1])],
                           np.array([0, offsets[where["tail"][0] + 1] - offsets[where["tail"][0]]], np.uint64)),
                       n_small: (codes, offsets)}
            for n in (300, 6000):
                batches[n] = concat_batches((codes, offsets), random_batch(leng + n, n - n_small, 0, lmax))
            info = assert_msv_plans_cover(e, leng, batches)
            ran = set()
            for n, (bc, bo) in batches.items():
                assert len(bo) - 1 == n
                w = want if n == n_small else (want[where["tail"][:1]] if n == 1 else o.score_batch(bc, bo, threads=8))
                ran.add(e.variant_for(n))
                assert same(e.score_batch(codes=bc, offsets=bo), w, f"LENG {leng} n {n} {e.variant_for(n)} host"), (leng, n)
                if n <= 300:
                    assert same(device_scores(e, bc, bo, longest_first=n == 300), w,
                                f"LENG {leng} n {n} {e.variant_for(n)} device"), (leng, n)
            if coop:
                assert coop in ran, (leng, coop, ran)
            print(f"LENG {leng}: plans {sorted(ran)}, main {info['variant']}")
        finally:
            e.close()
        for isc in (False, True):
            if cap not in VIT_CAPACITIES[isc]:
                continue
            mode = 1 if isc else 0
            v = msv.Viterbi_HMM(h, insert_mode=mode)
            try:
                vi = v.describe()
                assert 64 * vi["states_per_lane"] * vi["waves_per_sequence"] >= leng, (leng, vi["variant"])
                s, w, i = vit_layout(vi["variant"])
                assert (s, w, i) == (vi["states_per_lane"], vi["waves_per_sequence"], isc)
                vc, vo, _, vwant = aimed(leng, vit_boundaries(vi["variant"]), tmp_path_factory, True, mode)
                vc, vo = concat_batches((vc, vo), random_batch(leng + 1, 300 - (len(vo) - 1), 0, 130))
                full = np.concatenate([vwant, o.vit_score_batch(*_tail_of(vc, vo, len(vwant)), mode, threads=8)])
                assert same(v.score_batch(codes=vc, offsets=vo), full, f"LENG {leng} {vi['variant']}"), (leng, mode)
            finally:
                v.close()


def _tail_of(codes, offsets, first):
    """The sequences first .. n - 1 of a CSR batch, rebased."""
    o = offsets[first:] - offsets[first]
    return codes[int(offsets[first]):], o.astype(np.uint64)


# ---------------------------------------------------------------------------------------------------------
# 3. fused grid layouts over exact-fit profiles
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lengs", [(448, 960, 1464, 2480), (1536, 2432, 3072, 4096)], ids=["coop_fused", "fused"])
def test_score_grid_over_exact_fit_profiles(lengs, tmp_path_factory):
    """One score_grid call over exact-fit profiles of different variants with the same batch: every profile's
    table re-laid in the layout of the grid's largest model (the cooperative layout of 2480 states:
    coop_fused; the latency layout of 4096: Plan fused).  The batch holds tail and window homologs of every
    profile of the grid."""
    models = [model(leng, tmp_path_factory) for leng in lengs]
    parts = []
    for leng, (_, h, _) in zip(lengs, models):
        parts.append(tail_homolog_batch(h.match_emissions, 300 + leng, 4, 1, 130))
        parts.append(window_homolog_batch(h.match_emissions, 301 + leng, [leng // 2 - 12, leng - 40], 24))
        parts.append(random_batch(302 + leng, 2, 0, 130))
    codes, offsets = concat_batches(*parts)
    n = len(offsets) - 1
    engines = [msv.MSV_HMM(h) for _, h, _ in models]
    try:
        infos = [e.describe() for e in engines]
        if max(lengs) <= max(COOP_STATES.values()):
            # the rule of the fused cooperative launch (msv_plan.cpp fused_grid)
            assert all(i["coop_variant"] for i in infos) and len(engines) * n <= min(i["coop_max_n"] for i in infos)
        else:
            assert len(engines) * n <= 2048 and not infos[-1]["coop_variant"]
        grid = msv.score_grid(engines, codes=codes, offsets=offsets)
        assert grid.shape == (len(lengs), n)
        for k, (leng, (_, _, o)) in enumerate(zip(lengs, models)):
            assert same(grid[k], o.score_batch(codes, offsets), f"grid row LENG {leng}"), (lengs, leng)
    finally:
        for e in engines:
            e.close()


# ---------------------------------------------------------------------------------------------------------
# 4. tables with a state knocked out (-inf inside the model)
# ---------------------------------------------------------------------------------------------------------
def raw_msv_scores(p, codes, offsets):
    out = np.zeros(len(offsets) - 1, np.float32)
    st = _native.lib().msv_score_batch(p, codes.ctypes.data if codes.size else None, offsets.ctypes.data,
                                       len(offsets) - 1, out.ctypes.data, None)
    assert st == 0, st
    return out


def raw_vit_scores(p, codes, offsets):
    out = np.zeros(len(offsets) - 1, np.float32)
    st = _native.lib().msv_vit_score_batch(p, codes.ctypes.data if codes.size else None, offsets.ctypes.data,
                                           len(offsets) - 1, out.ctypes.data, None)
    assert st == 0, st
    return out


@pytest.mark.parametrize("name", ["msv_g16_s88_w16_p2_d1", "msv_g32_s76_a64_w16_p2_d1", "msv_g64_s64_w12_p2_d1"],
                         ids=["g16", "split", "big"])
def test_knocked_out_state_matches_the_cpu_dp(name, tmp_path_factory):
    """msv_profile_create / msv_vit_profile_create from a raw exact-fit table with one real column set to -inf --
    the last state, then the last state of a middle lane (whose M feeds shift_in) -- against the CPU DPs over
    the same table: under the automatic plans (one sequence, the batch) and the forced variant.  The only
    coverage of -inf emissions inside a model; the scores must also differ from the intact table's."""
    L = _native.lib()
    g, s, sa = msv_layout(name)
    leng = g * s
    _, h, o = model(leng, tmp_path_factory)
    es, consts, tsc = o.emission_scores(), o.constants(), o.vit_tables(0)[1]
    boundary = (g // 2) * s  # last state of lane G/2 - 1
    (codes, offsets), where = boundary_batch(h.match_emissions, 77 + leng, [boundary, boundary + sa], viterbi=True)
    intact = o.score_batch(codes, offsets)
    assert np.array_equal(bits(numpy_msv(es, *consts, codes, offsets)), bits(intact))
    for state in (leng, boundary):
        ko = knock_out(es, state)
        want = numpy_msv(ko, *consts, codes, offsets)
        vwant = vit_score_tables(ko, None, tsc, consts, codes, offsets)
        aimed_at = where["tail"] if state == leng else where["window"]
        # (the CPU figure is half or more of the tail homologs, test_state_batches.py; a quarter at these seeds)
        assert (bits(want)[aimed_at] != bits(intact)[aimed_at]).sum() * 4 >= len(aimed_at), (name, state)
        p = C.c_void_p()
        assert L.msv_profile_create(0, ko.ctypes.data, leng + 1, *consts, C.byref(p)) == 0
        try:
            assert same(raw_msv_scores(p, codes, offsets), want, f"{name} knocked {state} auto"), (name, state)
            one = where["tail"][0] if state == leng else where["window"][0]
            oc, oo = codes[int(offsets[one]):int(offsets[one + 1])], np.array([0, offsets[one + 1] - offsets[one]], np.uint64)
            assert bits(raw_msv_scores(p, oc, oo))[0] == bits(want)[one], (name, state)
            assert L.msv_profile_set_variant(p, name.encode()) == 0
            assert same(raw_msv_scores(p, codes, offsets), want, f"{name} knocked {state} forced"), (name, state)
        finally:
            L.msv_profile_destroy(p)
        p = C.c_void_p()
        tsc32 = np.ascontiguousarray(tsc, np.float32)
        assert L.msv_vit_profile_create(0, ko.ctypes.data, None, tsc32.ctypes.data, leng + 1, *consts, C.byref(p)) == 0
        try:
            assert same(raw_vit_scores(p, codes, offsets), vwant, f"{name} knocked {state} Viterbi"), (name, state)
        finally:
            L.msv_vit_profile_destroy(p)
