"""Models and batches for the four domain stages where most lanes hold no state (test helper; not a conftest).

dom_kernel.hip, aln_kernel.hip, aln_null2.hip and spl_kernel.hip run one item per 64-lane wave, lane l holding the S
states l S + 1 .. l S + S (S = 2, 6, 12, 22, 38).  The library gives a model the smallest S that holds it, so a model
at the low end of a variant's range leaves more than half of the wave to padding; the stages' own GPU suites force
every variant onto models that nearly fill it.  sparse_lengths(S) are the three lengths per S at which the padding
matters most, sparse_batch() applies the existing aimed builders (forward_batches, split_lib) to such a model, and
tests/test_sparse_lane_batches.py shows on the float64 twins that the batches reach the model's end, the last real
lane's boundary, a rescaled row and a two-segment sample.  Built on the host only."""
from __future__ import annotations

import functools

import numpy as np

from hmm_fasta_viterbi_amd.synthetic import concat_batches, random_batch
from forward_batches import aimed_batch, base_model, insertion_batch, rescaled_chain
from null2_lib import BLOCK_EDGES, LONGEST, R, cpu_null2, stretch, take
from split_lib import copies_batch
from state_batches import _csr

SLOTS = (2, 6, 12, 22, 38)
KINDS = ("first", "lane 32 alone", "ends a lane")
BLOCKS = (1, 2, 64, 65, 129)  # the residue-block edges of the decode, align and split suites
NULL2_BLOCKS = BLOCK_EDGES + (LONGEST,)  # those of the null2 suite: the edges of its row blocks


def sparse_lengths(S: int):
    """(first, lane 32 alone, ends a lane): 64 S' + 1, the first model the automatic choice gives this S (S' the next
    smaller size; LENG 3 at S = 2); 32 S + 1, node LENG alone in the first slot of lane 32, the only source lane of
    the scans' 32-lane step; 17 S, node LENG in the last slot of lane 16, the only source lane of the 16-lane step."""
    at = SLOTS.index(S)
    return (64 * SLOTS[at - 1] + 1 if at else 3, 32 * S + 1, 17 * S)


def lanes_used(leng: int, S: int) -> int:
    """How many of the 64 lanes hold a state of the model."""
    return (leng - 1) // S + 1


def larger(S: int):
    """The next larger S, None at 38."""
    at = SLOTS.index(S)
    return SLOTS[at + 1] if at + 1 < len(SLOTS) else None


def sparse_model(S: int, inserts: bool, which: int):
    """forward_batches.base_model at sparse_lengths(S)[which], seed 71 + which.  The LENG 3 model has seed 93: a hit
    of three states gains little more than B -> M, E -> J and the move cost it, so what a rescaled chain of 80 hits
    (240 residues) scores hangs on how sharp the model's one middle state was drawn.  93 is the first seed
    from 71 on whose chain passes 120 nats in float64 with and without insert odds (136 and 140; seed 71 gives 87 and
    83), searched on the CPU twin alone, so that the 5 x 22.2 nats tests/test_sparse_lane_batches.py asks of every
    model are cleared by more than another libm's last bits."""
    leng = sparse_lengths(S)[which]
    return base_model(leng, 93 if leng == 3 else 71 + which, inserts)


def sparse_batch(model, S: int, blocks=BLOCKS, cut=(20, 90)):
    """(codes, offsets, items, where): every fourth tail and head homolog and every window homolog of
    aimed_batch(model, S, 32) -- its windows cross the lane boundaries inside the model and the last real lane's --,
    every other sequence of insertion_batch(model, S, 42), one rescaled chain, the two-copy sequence and its control of
    split_lib.copies_batch(model), consensus stretches of exactly `blocks` residues; every non-empty sequence whole,
    then the envelope `cut` from the middle of the last stretch (i_from > 1, Lc > Le).  A model too short for the aimed
    batches (LENG < 24) has uniform sequences in their place.  where = {"chain", "two", "control"}: sequence indices
    (every sequence is non-empty, so they are item indices too)."""
    leng = model[0].shape[1] - 1
    if leng >= 24:
        (aimed, at), (ins, _) = aimed_batch(model, S, 32), insertion_batch(model, S, 42)
        pick = np.concatenate([at["tail"][::4], at["head"][::4], at.get("window", np.zeros(0, np.int64))])
        core = concat_batches(take(aimed, pick.astype(np.int64)), take(ins, range(0, len(ins[1]) - 1, 2)))
    else:
        core = random_batch(33, 6, 1, 40)
    run = min(20, leng)
    chain = rescaled_chain(model, 80, copies=240 // run, core=run)  # 240 residues, as the default 12 x 20
    copies = copies_batch(model)[0]
    codes, offsets = concat_batches(core, _csr([chain]), copies,
                                    _csr([stretch(model, L, 600 + L) for L in blocks]))
    n = len(offsets) - 1
    L = np.diff(offsets.astype(np.int64))
    assert L.min() > 0
    items = [(s, 1, int(L[s])) for s in range(n)]
    items.append((n - 1, *cut))
    first = len(core[1]) - 1
    return codes, offsets, items, {"chain": first, "two": first + 1, "control": first + 2}


@functools.lru_cache(maxsize=None)
def case(S: int, inserts: bool, which: int):
    """(model, codes, offsets, items, where) of one sparse model; computed once and shared: do not modify."""
    model = sparse_model(S, inserts, which)
    return (model, *sparse_batch(model, S))


def null2_refs(model, codes, offsets, items, bad=None):
    """[(null2, domcorrection) of msv_aln_cpu_null2 per item; None for item `bad`], as null2_lib.case makes them."""
    off = offsets.astype(np.int64)
    refs = []
    for q, (s, a, b) in enumerate(items):
        if q == bad:
            refs.append(None)
            continue
        st, n2, dc = cpu_null2(model, codes[off[s] + a - 1:off[s] + b], int(off[s + 1] - off[s]))
        assert st == 0
        refs.append((n2, dc))
    return refs


def with_spoiled(model, codes, offsets, items):
    """The batch with one more sequence, a stretch of R + 5 residues with one residue outside the 20, and its whole
    item last (null2_lib.null2_items' bad item).  Returns (codes, offsets, items, bad)."""
    spoiled = stretch(model, R + 5, 977).copy()
    spoiled[R + 1] = 21
    codes, offsets = concat_batches((codes, offsets), _csr([spoiled]))
    n = len(offsets) - 1
    return codes, offsets, list(items) + [(n - 1, 1, R + 5)], len(items)


@functools.lru_cache(maxsize=None)
def null2_case(S: int, inserts: bool, which: int):
    """(model, codes, offsets, items, bad, refs) for the null2 checks: sparse_batch with the null2 suite's block edges
    and its cut (rows R - 4 .. 3 R + 1 of the longest: no block of it starts where one did), then the bad item.
    Computed once and shared: do not modify."""
    model = sparse_model(S, inserts, which)
    codes, offsets, items, _ = sparse_batch(model, S, NULL2_BLOCKS, (R - 3, 3 * R + 2))
    codes, offsets, items, bad = with_spoiled(model, codes, offsets, items)
    return model, codes, offsets, items, bad, null2_refs(model, codes, offsets, items, bad)
