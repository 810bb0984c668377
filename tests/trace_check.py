"""An independent checker of Viterbi traces (test helper; not a conftest): is a reported path a legal path of
the model, and what does it score when its terms are summed left to right in float32 -- N loops, move, tBM, the
ops, then E->J or E->C, loops, move, the order of test_viterbi_paths.best_path.  No DP, no matrices: the DP's
value is the max over paths of exactly this sum, so the re-score of an optimal path has the score's bits.

Also the batches and the wrappers the trace tests share."""
from __future__ import annotations

import ctypes as C

import numpy as np

import hmm_fasta_viterbi_amd as msv
from hmm_fasta_viterbi_amd import _cpu_trace, _native
from state_batches import _cdf, _csr, _emit

F = np.float32
NINF = F(-np.inf)
MM, MI, MD, IM, II, DM, DD = range(7)
# transition (previous state, this state) -> column, read at the PREVIOUS state's node
TRANSITION = {("M", "M"): MM, ("M", "I"): MI, ("M", "D"): MD, ("I", "M"): IM, ("I", "I"): II, ("D", "M"): DM,
              ("D", "D"): DD}


def cpu_trace(msc, isc, tsc, consts, codes):
    """(score, [(i_from, i_to, k_from, k_to, ops bytes)]) of msv_vit_cpu_trace; asserts MSV_OK."""
    st, sc, doms, ops = _cpu_trace(msc, isc, tsc, consts, codes)
    assert st == 0, st
    return sc, domain_list(doms, ops)


def domain_list(doms, ops, base=0):
    return [(int(d["i_from"]), int(d["i_to"]), int(d["k_from"]), int(d["k_to"]),
             ops[int(d["ops_begin"]) - base:int(d["ops_begin"]) - base + int(d["ops_len"])].tobytes()) for d in doms]


def traces_lists(t):
    """Per entry of a Traces: its domains as domain_list gives them."""
    return [domain_list(t.domains_of(q), t.ops) for q in range(len(t))]


def check_legal(doms, leng, L):
    """Asserts that the domains describe a legal path: each starts and ends in M, no I at node LENG, no D at the
    exit, i and k in range and consistent with the ops, domains ordered and disjoint in i."""
    last_i = 0
    for (i_from, i_to, k_from, k_to, ops) in doms:
        assert len(ops) >= 1 and ops[0] == 77 and ops[-1] == 77, ops  # domain ends are M (D never exits)
        assert last_i < i_from <= i_to <= L, (last_i, i_from, i_to, L)
        assert 1 <= k_from <= k_to <= leng
        i, k = i_from - 1, k_from - 1
        for op in ops:
            assert op in (77, 73, 68), op
            if op == 77:
                i, k = i + 1, k + 1
            elif op == 73:
                i += 1
                assert k < leng, "I at node LENG"
            else:
                k += 1
            assert 1 <= i <= L and 1 <= k <= leng, (i, k)
        assert (i, k) == (i_to, k_to), ((i, k), (i_to, k_to))
        last_i = i_to


def rescore(msc, isc, tsc, consts, codes, doms):
    """The float32 left-to-right score of the path the domains describe (-inf for no domains: no path)."""
    tBM, tEC, tEJ = (F(x) for x in consts)
    L = len(codes)
    if not doms:
        return NINF
    loop, move = (F(x) for x in msv.sequence_transitions(L))
    s, at = F(0.0), 0  # N(0) = 0; `at` = residues emitted so far
    for n, (i_from, i_to, k_from, k_to, ops) in enumerate(doms):
        for _ in range(i_from - 1 - at):  # N or J loops
            s = F(s + loop)
        s = F(F(s + move) + tBM)          # -> B -> M(k_from)
        i, k, prev = i_from - 1, k_from - 1, None
        for op in ops:
            state = chr(op)
            if prev is not None:
                s = F(s + tsc[k, TRANSITION[(prev, state)]])
            if state == "M":
                i, k = i + 1, k + 1
                s = F(s + msc[codes[i - 1], k])
            elif state == "I":
                i += 1
                if isc is not None:
                    s = F(s + isc[codes[i - 1], k])
            else:
                k += 1
            prev = state
        at = i_to
        s = F(s + (tEJ if n + 1 < len(doms) else tEC))  # E -> J, or E -> C after the last domain
    for _ in range(L - at):
        s = F(s + loop)
    return F(s + move)


def tables_of(vit):
    """(msc, isc or None, tsc, consts) of a Viterbi_HMM, as the C calls take them."""
    return (vit.match_scores, vit.insert_scores if vit.insert_mode else None, vit.transition_scores,
            (vit.tr_B_Mk, vit.tr_E_C, vit.tr_E_J))


def cpu_traces(tables, codes, offsets, select=None):
    """[(score, domains)] of the CPU trace for the selected sequences of a CSR batch."""
    idx = range(len(offsets) - 1) if select is None else select
    return [cpu_trace(*tables, codes[int(offsets[s]):int(offsets[s + 1])]) for s in idx]


def assert_same(t, want, what=""):
    """A Traces against cpu_traces' list: score bits, domains and ops."""
    got = traces_lists(t)
    assert len(got) == len(want), what
    for q, (sc, doms) in enumerate(want):
        assert np.float32(t.scores[q]).view(np.uint32) == np.float32(sc).view(np.uint32), (what, q, t.scores[q], sc)
        assert got[q] == doms, (what, q, got[q], doms)


def two_core_batch(match_emissions, seed, n, core=24, spacer=(4, 12), sharpen=3.0, mutate=0.05):
    """n sequences, each two cores emitted by two windows of `core` states at random places of the model with a
    uniform spacer between them and uniform flanks: the best path of such a sequence usually has two domains."""
    rng = np.random.Generator(np.random.PCG64(seed))
    cdf = _cdf(match_emissions, sharpen)
    leng = cdf.shape[0]
    core = min(core, leng)
    seqs = []
    for _ in range(n):
        parts = [rng.integers(0, 20, size=int(rng.integers(0, 5)), dtype=np.uint8)]
        for half in range(2):
            start = int(rng.integers(0, leng - core + 1))
            parts.append(_emit(rng, cdf, start, core, mutate))
            gap = int(rng.integers(spacer[0], spacer[1] + 1)) if half == 0 else int(rng.integers(0, 5))
            parts.append(rng.integers(0, 20, size=gap, dtype=np.uint8))
        seqs.append(np.concatenate(parts))
    return _csr(seqs)


def profile_from_tables(msc, isc, tsc, consts, device=0):
    """msv_vit_profile_create over tables -> an object with Viterbi_HMM's trace and score calls."""
    vit = msv.Viterbi_HMM.__new__(msv.Viterbi_HMM)
    vit.model_length = msc.shape[1]
    vit.insert_mode = 0 if isc is None else 1
    vit.match_scores = np.ascontiguousarray(msc, np.float32)
    vit.insert_scores = np.zeros_like(vit.match_scores) if isc is None else np.ascontiguousarray(isc, np.float32)
    vit.transition_scores = np.ascontiguousarray(tsc, np.float32)
    vit.tr_B_Mk, vit.tr_E_C, vit.tr_E_J = (float(x) for x in consts)
    p = C.c_void_p()
    st = _native.lib().msv_vit_profile_create(device, vit.match_scores.ctypes.data,
                                              None if isc is None else vit.insert_scores.ctypes.data,
                                              vit.transition_scores.ctypes.data, vit.model_length, vit.tr_B_Mk,
                                              vit.tr_E_C, vit.tr_E_J, C.byref(p))
    assert st == 0, st
    vit._p = p
    vit.device = device
    return vit
