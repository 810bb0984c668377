"""Batches whose scores depend on chosen model states (test helper; not a conftest).

homolog_batch starts its core at a uniform random state, so on a model of a thousand states or more the best
path of a short sequence essentially never runs through the last states of the model: a kernel that drops,
misplaces or leaks the top state of its lane layout scores such a batch correctly.  The batches here aim the
emitted core at chosen states instead -- the last ones (tail_homolog_batch, tail_gapped_batch) or a window
across a lane, wave or table boundary (window_homolog_batch) -- and numpy_msv / oracle_lib.vit_score_tables
score a batch over a caller's table, so a column can be knocked out (set to -inf) to show that a batch's
scores depend on it.
"""
from __future__ import annotations

import numpy as np

import hmm_fasta_viterbi_amd as msv
from hmm_fasta_viterbi_amd.synthetic import random_batch

EDGE_LENGTHS = (0, 1, 2, 63, 64, 65)


def _cdf(match_emissions: np.ndarray, sharpen: float = 1.0) -> np.ndarray:
    probs = np.asarray(match_emissions, np.float64)[1:] ** sharpen
    return np.cumsum(probs / probs.sum(axis=1, keepdims=True), axis=1)


def _emit(rng, cdf: np.ndarray, start: int, core: int, mutate: float) -> np.ndarray:
    """One residue from each of the states start+1 .. start+core, a `mutate` fraction replaced by uniform ones
    (the draws of synthetic.homolog_batch, in its order)."""
    u = rng.random(core)
    emitted = np.minimum((cdf[start:start + core] < u[:, None]).sum(axis=1), 19).astype(np.uint8)
    flip = rng.random(core) < mutate
    emitted[flip] = rng.integers(0, 20, size=int(flip.sum()), dtype=np.uint8)
    return emitted


def _csr(seqs) -> tuple[np.ndarray, np.ndarray]:
    offsets = np.zeros(len(seqs) + 1, np.uint64)
    np.cumsum([len(s) for s in seqs], out=offsets[1:])
    codes = np.concatenate(seqs).astype(np.uint8) if len(seqs) and offsets[-1] else np.zeros(0, np.uint8)
    return codes, offsets


def _end_homolog_batch(match_emissions: np.ndarray, seed: int, n: int, lmin: int, lmax: int, mutate: float,
                       head: bool) -> tuple[np.ndarray, np.ndarray]:
    rng = np.random.Generator(np.random.PCG64(seed))
    cdf = _cdf(match_emissions)
    leng = cdf.shape[0]
    seqs = []
    for _ in range(n):
        L = int(rng.integers(lmin, lmax + 1))
        core = min(L, leng, int(rng.integers(max(1, L // 2), L + 1)))
        emitted = _emit(rng, cdf, 0 if head else leng - core, core, mutate)
        left = int(rng.integers(0, L - core + 1))
        seq = rng.integers(0, 20, size=L, dtype=np.uint8)
        seq[left:left + core] = emitted
        seqs.append(seq)
    return _csr(seqs)


def tail_homolog_batch(match_emissions: np.ndarray, seed: int, n: int, lmin: int, lmax: int,
                       mutate: float = 0.1) -> tuple[np.ndarray, np.ndarray]:
    """synthetic.homolog_batch with the core's end pinned to the LAST state: a sequence of length U[lmin, lmax]
    (lmin >= 1) whose core of U[L/2, L] residues (at most LENG) is emitted by the states LENG - core + 1 .. LENG,
    wrapped in uniform flanks."""
    return _end_homolog_batch(match_emissions, seed, n, lmin, lmax, mutate, head=False)


def head_homolog_batch(match_emissions: np.ndarray, seed: int, n: int, lmin: int, lmax: int,
                       mutate: float = 0.1) -> tuple[np.ndarray, np.ndarray]:
    """tail_homolog_batch mirrored: the core's START pinned to state 1 (emitted by the states 1 .. core)."""
    return _end_homolog_batch(match_emissions, seed, n, lmin, lmax, mutate, head=True)


def window_homolog_batch(match_emissions: np.ndarray, seed: int, starts, core: int, mutate: float = 0.1,
                         flank: int = 6, sharpen: float = 3.0) -> tuple[np.ndarray, np.ndarray]:
    """One sequence per entry of `starts`: a core emitted by the states start+1 .. start+core (clipped to
    1 .. LENG) between uniform flanks of U[0, flank] residues.  With start = b - core / 2 the core straddles
    the boundary between states b and b + 1.  A window has one short sequence to put its path through the
    chosen states, so each state emits from its distribution raised to the power `sharpen` (renormalised;
    1 = the distribution itself): at 1 one 24-state core in five scored below an unrelated diagonal of a
    1408-state model and missed its states."""
    rng = np.random.Generator(np.random.PCG64(seed))
    cdf = _cdf(match_emissions, sharpen)
    leng = cdf.shape[0]
    seqs = []
    for start in starts:
        lo = max(0, min(int(start), leng - 1))
        hi = max(lo + 1, min(int(start) + core, leng))
        emitted = _emit(rng, cdf, lo, hi - lo, mutate)
        left, right = (int(x) for x in rng.integers(0, flank + 1, size=2))
        seqs.append(np.concatenate([rng.integers(0, 20, size=left, dtype=np.uint8), emitted,
                                    rng.integers(0, 20, size=right, dtype=np.uint8)]))
    return _csr(seqs)


def window_core(start: int, core: int, leng: int) -> tuple[int, int]:
    """(first, last) state of the core window_homolog_batch emits for `start` on a model of LENG `leng`."""
    lo = max(0, min(int(start), leng - 1))
    return lo + 1, max(lo + 1, min(int(start) + core, leng))


def tail_gapped_batch(match_emissions: np.ndarray, seed: int, n: int, lmin: int, lmax: int, p_delete: float = 0.06,
                      max_delete: int = 12, p_insert: float = 0.03, max_insert: int = 4,
                      mutate: float = 0.05, sharpen: float = 3.0) -> tuple[np.ndarray, np.ndarray]:
    """synthetic.gapped_homolog_batch walked BACKWARDS from the last node: the path ends in node LENG (emitted
    by M(LENG), or skipped so that a D chain runs into it) and reaches down with deletions of 1..max_delete
    nodes and insertions of 1..max_insert uniform residues until its U[L/2, L] residues are emitted; uniform
    flanks around the core.  The states emit from their sharpened distributions (window_homolog_batch): a path
    that pays for its gaps has to beat the ungapped diagonals elsewhere in the model."""
    rng = np.random.Generator(np.random.PCG64(seed))
    cdf = _cdf(match_emissions, sharpen)
    leng = cdf.shape[0]
    seqs = []
    for _ in range(n):
        L = int(rng.integers(lmin, lmax + 1))
        target = int(rng.integers(max(1, L // 2), L + 1))
        k = leng - 1  # index of node LENG
        if rng.random() < 0.5:  # the path's last nodes are deleted: D(.. LENG)
            k -= int(rng.integers(1, max_delete + 1))
        core = []  # built from the end
        while k >= 0 and len(core) < target:
            u = rng.random()
            if u < p_delete and core:
                k -= int(rng.integers(1, max_delete + 1))
                continue
            if u < p_delete + p_insert and core:
                core.extend(rng.integers(0, 20, size=int(rng.integers(1, max_insert + 1))).tolist())
            x = int(min((cdf[k] < rng.random()).sum(), 19))
            core.append(int(rng.integers(0, 20)) if rng.random() < mutate else x)
            k -= 1
        core = np.array(core[::-1][-L:], np.uint8)
        left = int(rng.integers(0, L - len(core) + 1))
        seq = rng.integers(0, 20, size=L, dtype=np.uint8)
        seq[left:left + len(core)] = core
        seqs.append(seq)
    return _csr(seqs)


def edge_batch(seed: int) -> tuple[np.ndarray, np.ndarray]:
    """Uniform sequences of the edge lengths 0, 1, 2, 63, 64, 65."""
    rng = np.random.Generator(np.random.PCG64(seed))
    return _csr([rng.integers(0, 20, size=L, dtype=np.uint8) for L in EDGE_LENGTHS])


def interleave(kinds, fill) -> tuple[tuple[np.ndarray, np.ndarray], dict]:
    """The sequences of the CSR batches `kinds` ({name: batch}) in order, each followed by the next sequence of
    `fill` while it lasts (then the rest of `fill`): neighbours in the queue share a wave, so a leak out of an
    aimed sequence lands on a sequence that shows it.  Returns the batch and {name: indices in it}."""
    fc, fo = fill
    seqs, where, f = [], {name: [] for name in kinds}, 0
    for name, (c, o) in kinds.items():
        for i in range(len(o) - 1):
            where[name].append(len(seqs))
            seqs.append(c[int(o[i]):int(o[i + 1])])
            if f < len(fo) - 1:
                seqs.append(fc[int(fo[f]):int(fo[f + 1])])
                f += 1
    for i in range(f, len(fo) - 1):
        seqs.append(fc[int(fo[i]):int(fo[i + 1])])
    return _csr(seqs), {k: np.array(v, np.int64) for k, v in where.items()}


def boundary_batch(match_emissions: np.ndarray, seed: int, boundaries, viterbi: bool = False, core: int = 24,
                   lmax: int = 130):
    """The batch of the capacity-edge tests for a model: one window homolog across each state boundary
    b | b + 1 of `boundaries` that lies inside the model, 24 tail homologs (lengths 1..lmax), for Viterbi 12 gapped
    sequences whose path ends in the last nodes, the edge lengths, and 24 uniform sequences interleaved
    between them.  Returns ((codes, offsets), {kind: indices})."""
    leng = np.asarray(match_emissions).shape[0] - 1
    starts = sorted({max(0, int(b) - core // 2) for b in boundaries if 1 <= int(b) < leng})
    kinds = {}
    if starts:
        kinds["window"] = window_homolog_batch(match_emissions, seed + 1, starts, core)
    kinds["tail"] = tail_homolog_batch(match_emissions, seed, 24, 1, lmax)
    if viterbi:
        kinds["gapped"] = tail_gapped_batch(match_emissions, seed + 2, 12, 8, lmax)
    kinds["edge"] = edge_batch(seed + 3)
    return interleave(kinds, random_batch(seed + 4, 24, 1, lmax))


def numpy_msv(es, tBMk, tEC, tEJ, codes, offsets):
    """float32 restatement of MSV_HMM::run_on_sequence (MSV_HMM.cpp:74-113) with free tr_E_C /
    tr_E_J (the reference fixes both to logf(0.5f)); every add is one IEEE float32 op in the
    reference's order, max is exact, so results are bit-comparable."""
    f = np.float32
    out = np.zeros(len(offsets) - 1, np.float32)
    for s in range(len(offsets) - 1):
        seq = codes[int(offsets[s]):int(offsets[s + 1])]
        L = len(seq)
        loop, move = msv.sequence_transitions(L)
        loop, move = f(loop), f(move)
        M = np.full(es.shape[1], -np.inf, np.float32)
        J = C = f(-np.inf)
        N, B = f(0.0), move
        for r in seq:
            Bt = f(B + f(tBMk))
            newM = np.full_like(M, -np.inf)
            newM[1:] = es[r, 1:] + np.maximum(M[:-1], Bt)
            M = newM
            E = M[1:].max()
            J = max(f(J + loop), f(E + f(tEJ)))
            C = max(f(C + loop), f(E + f(tEC)))
            N = f(N + loop)
            B = f(max(N, J) + move)
        out[s] = f(C + move) if L else -np.inf
    return out


def knock_out(table: np.ndarray, state) -> np.ndarray:
    """A copy of a [20][M] score table with the column(s) of `state` (1 .. LENG; one or a list) set to -inf."""
    out = np.array(table, np.float32, copy=True)
    out[:, state] = -np.inf
    return out
