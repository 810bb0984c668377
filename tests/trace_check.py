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


class PyTrace:
    """py_trace's result: the score, the domains, per rule ("M", "I", "D", "E", "C", "J", "B") the number of
    on-path decisions that had two or more equal candidates, and per on-path E tie the tied nodes."""

    def __init__(self, score):
        self.score, self.domains = score, []
        self.ties = dict.fromkeys("MIDECJB", 0)
        self.e_tied = []

    @property
    def tied(self):
        return sum(self.ties.values()) > 0


def py_trace(msc, isc, tsc, consts, codes):
    """The trace by a plain float32 numpy DP that keeps the full matrices (msv.h "Viterbi traces"): the M and I
    rows vectorised, the D chain a scalar loop.  On the way back each source is found by comparing the cell's
    value before its emission with fl(pred + t) of every candidate, in msv.h's order; a decision with two or
    more equal candidates is counted as a tie of its rule."""
    tBM, tEC, tEJ = (F(x) for x in consts)
    K, L = msc.shape[1] - 1, len(codes)
    loop, move = (F(x) for x in msv.sequence_transitions(L))
    Mx, Ix, Dx = (np.full((L + 1, K + 1), NINF, F) for _ in range(3))
    N, B, J, Cc, E = (np.full(L + 1, NINF, F) for _ in range(5))
    N[0], B[0] = F(0.0), move
    tmm, tim, tdm, tmd, tdd = (np.ascontiguousarray(tsc[:K, c], F) for c in (MM, IM, DM, MD, DD))  # into node k from k-1
    with np.errstate(invalid="ignore"):
        for i in range(1, L + 1):
            r = int(codes[i - 1])
            bt = F(B[i - 1] + tBM)
            m = np.maximum(np.maximum(Mx[i - 1, :K] + tmm, Ix[i - 1, :K] + tim), np.maximum(Dx[i - 1, :K] + tdm, bt))
            Mx[i, 1:] = m + msc[r, 1:]
            if K > 1:
                iv = np.maximum(Mx[i - 1, 1:K] + tsc[1:K, MI], Ix[i - 1, 1:K] + tsc[1:K, II])
                Ix[i, 1:K] = iv if isc is None else iv + isc[r, 1:K]
            md = Mx[i, :K] + tmd  # md[k - 1] = M(i,k-1) + tMD of node k-1
            d = NINF
            row = Dx[i]
            for k in range(2, K + 1):
                d = max(md[k - 1], d + tdd[k - 1])
                row[k] = d
            E[i] = Mx[i, 1:].max()
            J[i] = max(F(J[i - 1] + loop), F(E[i] + tEJ))
            Cc[i] = max(F(Cc[i - 1] + loop), F(E[i] + tEC))
            N[i] = F(N[i - 1] + loop)
            B[i] = max(F(N[i] + move), F(J[i] + move))
    out = PyTrace(F(Cc[L] + move) if L else NINF)
    if L == 0 or not np.isfinite(out.score):
        return out

    def pick(rule, value, cands):
        """The first candidate (name, float) equal to `value`; counts a tie when more than one is."""
        hit = [name for name, c in cands if c == value]
        assert hit, (rule, value, cands)
        out.ties[rule] += len(hit) > 1
        return hit[0]

    i = L
    while pick("C", Cc[i], [("loop", F(Cc[i - 1] + loop)), ("E", F(E[i] + tEC))]) == "loop":
        i -= 1
    while True:
        nodes = np.flatnonzero(Mx[i, 1:] == E[i]) + 1
        if len(nodes) > 1:
            out.ties["E"] += 1
            out.e_tied.append(nodes)
        k = int(nodes[0])
        i_to, k_to, ops, st = i, k, [], "M"
        while True:
            ops.append(st)
            if st == "M":
                cands = [("M", F(Mx[i - 1, k - 1] + tsc[k - 1, MM])), ("I", F(Ix[i - 1, k - 1] + tsc[k - 1, IM])),
                         ("D", F(Dx[i - 1, k - 1] + tsc[k - 1, DM])), ("B", F(B[i - 1] + tBM))]
                src = pick("M", max(c for _, c in cands), cands)
                i, k = i - 1, k - 1
                if src == "B":
                    break
                st = src
            elif st == "I":
                cands = [("M", F(Mx[i - 1, k] + tsc[k, MI])), ("I", F(Ix[i - 1, k] + tsc[k, II]))]
                st = pick("I", max(c for _, c in cands), cands)
                i -= 1
            else:
                st = pick("D", Dx[i, k], [("M", F(Mx[i, k - 1] + tsc[k - 1, MD])), ("D", F(Dx[i, k - 1] + tsc[k - 1, DD]))])
                k -= 1
        out.domains.append((i + 1, i_to, k + 1, k_to, "".join(reversed(ops)).encode()))
        if i == 0 or pick("B", B[i], [("N", F(N[i] + move)), ("J", F(J[i] + move))]) == "N":
            break
        while pick("J", J[i], [("loop", F(J[i - 1] + loop)), ("E", F(E[i] + tEJ))]) == "loop":
            i -= 1
    out.domains.reverse()
    return out


def quantised_model(rng, leng, inserts, distinct_exits, step=0.5, emissions=None, depth=2.0, period=None):
    """A model whose every score is a multiple of `step` from a small range, so that sums of different terms
    coincide often: match scores from `emissions` (default: multiples of step in [-depth, depth / 2]), insert
    scores in [-1, 0], transitions, the entry and the exits in [-depth, 0].  With `period` the nodes repeat with
    that period (a low-complexity model): whole paths then tie with their shifted copies."""
    M = leng + 1
    grid = np.arange(-depth, depth / 2 + step / 2, step) if emissions is None else np.asarray(emissions, float)
    msc = rng.choice(grid, (20, M)).astype(F)
    msc[:, 0] = NINF
    isc = (-step * rng.integers(0, int(1 / step) + 1, (20, M))).astype(F) if inserts else None
    tsc = (-step * rng.integers(0, int(depth / step) + 1, (M, 7))).astype(F)
    if period:
        src = 1 + np.arange(leng) % period
        msc[:, 1:], tsc[1:] = msc[:, src], tsc[src]
        if inserts:
            isc[:, 1:] = isc[:, src]
    tBM = F(-step * rng.integers(1, int(depth / step) + 1))
    tEC = F(-step * rng.integers(0, int(depth / step) + 1))
    tEJ = F(tEC - step * rng.integers(1, 4)) if distinct_exits else tEC
    return msc, isc, tsc, (tBM, tEC, tEJ)


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
