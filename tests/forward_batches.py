"""Models and batches aimed at the Forward kernel's lane edges and scan steps (test helper; not a conftest).

The Forward stage is compared within a tolerance, not bitwise, so an error has to move a score by more than the
tolerance to be seen.  The models here are raw tables (msc [20][M], isc [20][M] or None, tsc [M][7], consts), made
from a seed with numpy and handed to forward_lib.create_profile / cpu_scores: sharp match columns, every transition
distinct per node (a value read from the neighbouring node, or for the wrong lane, is another value), informative
per-node insert scores for the insert-odds variants.  The kernel's layout (fwd_kernel.hip): lane l holds states
l S + 1 .. l S + S; the *_IN slot arrays hold node k-1's transition at state k; nodes 1 .. LENG-1 have transitions
and I states; D -> E exits run for k >= 2.

bridge_model / bridge_sequences put the score of a sequence on ONE long D chain whose length decides which step of
the cross-lane scan has to deliver it; aimed_batch aims cores at state 1, state LENG and the lane boundaries;
insertion_batch puts insertions into a lane's last and first slot; knocked() closes a node, so that the scan's
multipliers across it are exactly 0.  tests/test_forward_batches.py shows on the CPU that each aim is real.
"""
from __future__ import annotations

import numpy as np

from hmm_fasta_viterbi_amd.synthetic import random_batch
from state_batches import (_csr, edge_batch, head_homolog_batch, interleave, tail_homolog_batch,
                           window_homolog_batch)

MM, MI, MD, IM, II, DM, DD = range(7)
SCAN_STEPS = 6
# the lane boundaries 0|1, 15|16, 31|32, 62|63: boundary l-1 | l lies between the states l S and l S + 1
BOUNDARY_LANES = (1, 16, 32, 63)
INSERT_LANES = (1, 32, 63)


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def base_model(leng: int, seed: int, inserts: bool = False):
    """Sharp match columns (Dirichlet(0.3) rows -> log(20 p); states 1 and LENG sharper still: one residue at
    0.97), transitions distinct per node drawn from the ranges
    of synthetic.write_hmm (i->m and i->i, constants there, spread around its values), distinct exits, and with
    `inserts` a per-node insert table (Dirichlet(2) rows -> log(20 p)).  The rows of node 0 and node LENG are filled
    like every other: the model has no such transitions, so a builder that read them would show."""
    rng = _rng(seed)
    M = leng + 1
    p = rng.dirichlet(np.full(20, 0.3), size=M) + 1e-6
    p /= p.sum(axis=1, keepdims=True)
    for end in (1, leng):  # the end states stand alone beside a clipped window or insertion: one residue at 0.97
        best = int(np.argmax(p[end]))
        p[end] *= 0.03 / (1.0 - p[end, best])
        p[end, best] = 0.97
    msc = np.log(20.0 * p).T.astype(np.float32).copy()
    msc[:, 0] = -np.inf
    isc = None
    if inserts:
        isc = np.log(20.0 * rng.dirichlet(np.full(20, 2.0), size=M)).T.astype(np.float32).copy()
    cost = np.empty((M, 7))
    for col, (lo, hi) in {MM: (0.01, 0.1), MI: (3.5, 5.0), MD: (4.0, 6.0), IM: (0.5, 0.75), II: (0.65, 0.9),
                          DM: (0.3, 0.6), DD: (0.8, 1.2)}.items():
        cost[:, col] = rng.uniform(lo, hi, M)
    tsc = (-cost).astype(np.float32)
    consts = (float(np.float32(np.log(2.0 / (leng * (leng + 1.0))))), float(np.float32(np.log(0.5) - 0.75)),
              float(np.float32(np.log(0.5))))
    return msc, isc, tsc, consts


def emissions(model) -> np.ndarray:
    """[M][20] match-emission probabilities of a model (row 0 zeros), as Profile_HMM.match_emissions."""
    msc = model[0].astype(np.float64)
    with np.errstate(over="ignore"):
        me = np.exp(msc.T) / 20.0
    me[0] = 0.0
    return me


def consensus(model, first: int, last: int) -> np.ndarray:
    """The best-scoring residue of each state first .. last."""
    return np.argmax(model[0][:, first:last + 1], axis=0).astype(np.uint8)


# ---- bridges: one D chain per scan step -------------------------------------------------------------------------

def bridge_plan(S: int):
    """[(source node s_j, landing state k_j)] for the scan steps j = 0 .. 5 on a model of LENG 64 S.  Sources sit
    alternately in a lane's first and last slot, from lane 4 on (at least 8 states into the model at S = 2);
    landings alternate likewise with half the frequency, so that the four pairings occur.  The chain from D(s+1)
    to D(k-1) makes k - s - 2 d->d steps, more than S (2^j + 1): it crosses more than 2^j lane boundaries, so
    the scan's steps below j cannot deliver it."""
    plan = []
    for j in range(SCAN_STEPS):
        lane = 4 + 3 * j
        s = lane * S + 1 if j % 2 == 0 else lane * S + S
        k = s + S * (2 ** j + 1) + 3  # the first state far enough
        want_slot = 0 if (j // 2) % 2 == 0 else S - 1
        k += (want_slot - (k - 1) % S) % S
        assert k - s - 2 > S * (2 ** j + 1) and s >= 8 and k + 7 <= 64 * S - 8
        plan.append((s, k))
    return plan


def bridge_model(S: int, seed: int, inserts: bool = False):
    """LENG 64 S.  Deletions are rare to open and to close (m->d and d->m uniform in [0.005, 0.02] per node) and
    cheap to extend (d->d uniform in [0.999, 0.9999] per node: 0.5 of the mass survives 1,300 states); bridge j
    opens at its source (m->d 0.5) and closes at its landing (d->m of node k_j - 1 = 0.9).  About a quarter of the
    lanes, drawn, hold one toll node with d->d uniform in [0.7, 0.9]: with d->d that close to 1 everywhere the whole-
    lane products, and so the scan multipliers A[j] of neighbouring lanes, would differ by less than the tolerance
    can see; with the tolls they differ by 10-30 % wherever a window of lanes gains or loses a toll, and the lane
    left of each landing's lane holds one for certain.  The d->d into
    each bridge's last D state, D(k_j - 1), is a toll too: the prefix product c_q of that slot then differs as much
    from its neighbours', and the landing takes all it gets from upstream lanes through that one c_q."""
    leng = 64 * S
    msc, isc, tsc, consts = base_model(leng, seed, inserts)
    rng = _rng(seed + 1)
    M = leng + 1
    tsc[:, MD] = np.log(rng.uniform(0.005, 0.02, M)).astype(np.float32)
    tsc[:, DM] = np.log(rng.uniform(0.005, 0.02, M)).astype(np.float32)
    tsc[:, DD] = np.log(rng.uniform(0.999, 0.9999, M)).astype(np.float32)
    for lane in np.flatnonzero(rng.random(64) < 0.25):
        tsc[int(lane) * S + int(rng.integers(0, S)) + 1, DD] = np.float32(np.log(rng.uniform(0.7, 0.9)))
    for s, k in bridge_plan(S):
        # the lane left of the one the chain lands in is the top of the last scan step its mass takes: with a toll
        # there, that step's multiplier differs from the one a lane to its left or right would have given
        nodes = np.arange(((k - 2) // S - 1) * S + 1, ((k - 2) // S) * S + 1)
        if tsc[nodes, DD].min() > np.log(0.99):
            tsc[int(rng.choice(nodes)), DD] = np.float32(np.log(rng.uniform(0.7, 0.9)))
    for s, k in bridge_plan(S):
        tsc[s, MD] = np.float32(np.log(0.5))
        tsc[k - 1, DM] = np.float32(np.log(0.9))
        tsc[k - 2, DD] = np.float32(np.log(rng.uniform(0.7, 0.9)))  # the last step into D(k-1), the state that lands
    return msc, isc, tsc, consts


def bridge_sequences(model, S: int, seed: int, flank=None, cross: bool = False):
    """One sequence per bridge: `flank` (None: 0-3, drawn) uniform residues, the consensus of states s-7 .. s, the
    consensus of k .. k+7, `flank` uniform residues.  The only cheap path emits the first half up to the source,
    deletes to the landing and emits the second half.  `cross` gives the other pairings instead: the source of
    bridge i with the landing of bridge j != i wherever the landing lies at least 16 states downstream -- every
    pairing is a chain of its own length, so it takes its own route through the scan's steps and lanes."""
    rng = _rng(seed)
    plan = bridge_plan(S)
    pairs = [(s, k) for i, (s, _) in enumerate(plan) for j, (_, k) in enumerate(plan) if i != j and k >= s + 16] \
        if cross else plan
    seqs = []
    for s, k in pairs:
        left, right = (int(x) for x in rng.integers(0, 4, size=2)) if flank is None else (flank, flank)
        seqs.append(np.concatenate([rng.integers(0, 20, size=left, dtype=np.uint8), consensus(model, s - 7, s),
                                    consensus(model, k, k + 7), rng.integers(0, 20, size=right, dtype=np.uint8)]))
    return _csr(seqs)


# ---- the edges -----------------------------------------------------------------------------------------------------

def sharpened(me: np.ndarray, power: float = 3.0) -> np.ndarray:
    out = np.asarray(me, np.float64) ** power
    out[1:] /= out[1:].sum(axis=1, keepdims=True)
    return out


def boundary_states(leng: int, S: int):
    """The states b (boundary b | b + 1) of the lane boundaries 0|1, 15|16, 31|32, 62|63 and of the last real
    lane's boundary that lie inside the model."""
    last_lane = (leng - 1) // S
    return sorted({b for b in [lane * S for lane in BOUNDARY_LANES + (last_lane,)] if 1 <= b < leng})


def aimed_batch(model, S: int, seed: int, lmax: int = 130):
    """24 tail homologs whose core ends in state LENG and 24 head homologs whose core starts in state 1 (emitted
    from the distributions raised to the power 3, lengths 8 .. lmax), one 24-state window homolog across each of
    boundary_states() (power 6, no mutation: at S = 2 the first boundary has two states before it), the edge
    lengths 0, 1, 2, 63, 64, 65, and uniform sequences in between.
    Returns ((codes, offsets), {kind: indices})."""
    me = emissions(model)
    leng = me.shape[0] - 1
    sharp = sharpened(me)
    kinds = {"tail": tail_homolog_batch(sharp, seed, 24, 8, lmax),
             "head": head_homolog_batch(sharp, seed + 1, 24, 8, lmax)}
    bounds = boundary_states(leng, S)
    if bounds:
        kinds["window"] = window_homolog_batch(me, seed + 2, [max(0, b - 12) for b in bounds], 24, mutate=0.0,
                                               sharpen=6.0)
    kinds["edge"] = edge_batch(seed + 3)
    return interleave(kinds, random_batch(seed + 4, 30, 1, lmax))


def _insert_residues(model, node: int, n: int, rng) -> np.ndarray:
    """n residues that look like an insertion after `node`: drawn uniformly from the residues that score below -2
    nats at each of the match states node-1 .. node+2 (or the alternative that shifts the insertion to a
    neighbouring node and lets a match state emit one of them is nearly as good as the aimed path), and, with an
    insert table, from the better half of those by the node's own insert score."""
    msc, isc = model[0], model[1]
    leng = msc.shape[1] - 1
    near = msc[:, max(1, node - 1):min(leng, node + 2) + 1].max(axis=1)
    cand = np.flatnonzero(near < -2.0)
    if len(cand) < 4:
        cand = np.argsort(near, kind="stable")[:4]
    if isc is not None:
        cand = cand[np.argsort(-isc[cand, node], kind="stable")][:max(2, len(cand) // 2)]
    return cand[rng.integers(0, len(cand), size=n)].astype(np.uint8)


def _lone_state_pays(model, node: int, n: int) -> bool:
    """Node LENG - 1, n residues inserted, state LENG alone beyond: against ending the alignment in `node` and
    leaving the rest to the flank, the path through the I state weighs about exp(best match score of LENG + m->i
    + i->m + (n - 1) i->i) to 1.  True if closing it would move the score by 200 tolerances of msv.h
    (16 (L + LENG) 2^-24 at L = 30) or more."""
    msc, _, tsc, _ = model
    leng = msc.shape[1] - 1
    net = float(msc[:, leng].max()) + float(tsc[node, MI]) + float(tsc[node, IM]) + (n - 1) * float(tsc[node, II])
    return np.log1p(np.exp(net)) >= 200.0 * 16.0 * (leng + 30) * 2.0 ** -24


def insertion_batch(model, S: int, seed: int):
    """I states at the lane edges: for the lane boundaries 0|1, 31|32 and 62|63, the consensus of the 24 states
    around the boundary b | b + 1 (clipped to the model) with n = 1 .. 4 residues (_insert_residues) inserted after
    node b (a lane's last slot: the I state that the next lane's first M reads through the one-lane shift) and,
    likewise, after node b + 1 (the next lane's first slot, fed by the M that took its inputs through that shift);
    0-3 uniform residues around.  Nodes without an I state (>= LENG) are left out.  Where the model's end leaves
    fewer than 3 core states on one side of the insertion (S = 2, and the shortened models) the insertions are of
    1, 2, 1, 2 residues: dropping so short a side into the flank costs about what opening an insertion does, and
    every further inserted residue shifts the weight away from the I state.  Where a single state lies beyond the
    insertion (node LENG - 1) a sequence is made only if the model's own numbers let that state pay for the
    insertion by a margin the tolerance can see (_lone_state_pays): at S = 2 always, at S = 38 never.
    Returns ((codes, offsets), the node of each sequence)."""
    rng = _rng(seed)
    leng = model[0].shape[1] - 1
    seqs, nodes = [], []
    for lane in INSERT_LANES:
        b = lane * S
        first, last = max(1, b - 11), min(leng, b + 12)
        for node in (b, b + 1):
            if node >= leng or node < first:
                continue
            short = node - first + 1 < 3 or last - node < 3
            for n in ((1, 2, 1, 2) if short else (1, 2, 3, 4)):
                left, right = (int(x) for x in rng.integers(0, 4, size=2))
                if last - node == 1 and not _lone_state_pays(model, node, n):
                    continue
                seqs.append(np.concatenate([rng.integers(0, 20, size=left, dtype=np.uint8),
                                            consensus(model, first, node), _insert_residues(model, node, n, rng),
                                            consensus(model, node + 1, last),
                                            rng.integers(0, 20, size=right, dtype=np.uint8)]))
                nodes.append(node)
    return _csr(seqs), np.array(nodes, np.int64)


# ---- rescaled chains and deep queues -------------------------------------------------------------------------------

def rescaled_chain(model, seed: int, copies: int = 12, core: int = 20) -> np.ndarray:
    """`copies` consensus runs of `core` states from random starts, concatenated into one multi-hit sequence: a hit
    adds 18-25 nats and the kernel rescales whenever a row's E passes 2^32 (22 nats), so after a few hits the
    scale's exponent is far from 0 (the tests assert the reference score that shows it)."""
    rng = _rng(seed)
    leng = model[0].shape[1] - 1
    starts = rng.integers(1, leng - core + 2, size=copies)
    return np.concatenate([consensus(model, int(s), int(s) + core - 1) for s in starts])


def queue_batch(model, n: int, seed: int, lmax: int = 24):
    """n sequences for a queue deeper than the grid: a third homologs of length 1 .. lmax (distributions raised to
    the power 3), one rescaled chain of 4 hits (80 residues) in every 64 -- the wave that scores it carries a
    non-zero exponent to its next sequence unless it resets it -- and uniform sequences of length 0 .. lmax for the
    rest; shuffled.  Returns ((codes, offsets), the indices of the chains)."""
    from hmm_fasta_viterbi_amd.synthetic import concat_batches, homolog_batch
    from queue_batches import take_sequences
    rng = _rng(seed)
    n_chain, n_hom = max(1, n // 64), n // 3
    chains = _csr([rescaled_chain(model, seed + 3 + i, copies=4) for i in range(n_chain)])
    batch = concat_batches(chains, homolog_batch(sharpened(emissions(model)), seed + 1, n_hom, 1, lmax),
                           random_batch(seed + 2, n - n_chain - n_hom, 0, lmax))
    perm = rng.permutation(n)
    where = np.empty(n, np.int64)
    where[perm] = np.arange(n)
    return take_sequences(*batch, perm), np.sort(where[:n_chain])


# ---- zeros inside the model ----------------------------------------------------------------------------------------

def knocked(model, node: int):
    """A copy of the model with the match column and the d->d, m->d and d->m of `node` set to -inf: nothing passes
    the node, and every product of d->d across it is exactly 0."""
    msc, isc, tsc, consts = model
    msc, tsc = msc.copy(), tsc.copy()
    msc[:, node] = -np.inf
    tsc[node, [DD, MD, DM]] = -np.inf
    return msc, isc, tsc, consts


def with_transition(model, column: int, value, node=None):
    """A copy of the model with one transition column set to `value` at `node` (None: at every node)."""
    msc, isc, tsc, consts = model
    tsc = tsc.copy()
    tsc[slice(None) if node is None else node, column] = np.float32(value)
    return msc, isc, tsc, consts
