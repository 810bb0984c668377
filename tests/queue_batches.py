"""Batches deeper than a persistent grid (test helper; not a conftest).

Every kernel here runs a persistent grid: a wave, a lane group (MSV) or a team of waves (Viterbi) takes its
first sequence statically and every later one from an atomic counter, and the launchers never start more
workgroups than the batch needs.  So a batch no larger than the grid's capacity gives every stream exactly
one sequence, and the code that carries a stream from one sequence to the next never runs.  The capacities
below are upper bounds on the streams in flight: n > capacity proves by pigeonhole that some stream scores a
second sequence, n > 2 * capacity that some stream scores a third.

queue_batch() builds such a batch cheaply: the queue has to be deep, not long, so the sequences are short
(lengths U[1, lmax], lmax = 130 crosses the kernels' 64-row residue blocks twice), with profile-emitted
sequences (J overtakes N, D chains cross lanes) and the edge lengths spread through the whole queue.
"""
from __future__ import annotations

import re

import numpy as np

from hmm_fasta_viterbi_amd.synthetic import concat_batches, gapped_homolog_batch, homolog_batch, random_batch

EDGE_LENGTHS = (0, 1, 2, 3, 63, 64, 65, 127, 128, 129)
EDGE_COPIES = 40
HOMOLOGS = 1500  # of each kind (ungapped, gapped), at most an eighth of the batch each


def viterbi_capacity(info: dict) -> int:
    """Sequences a full Viterbi grid holds at once (Viterbi_HMM.describe()): one per wave, or per team."""
    return info["blocks"] * info["waves_per_block"] // info["waves_per_sequence"]


def msv_streams(name: str) -> int:
    """D of an MSV variant name msv_g<G>_s<S>..._d<D>: the sequences a lane group interleaves."""
    m = re.search(r"_d(\d+)$", name)
    if not m:
        raise ValueError(f"no _d<D> in {name!r}")
    return int(m.group(1))


def msv_groups(info: dict) -> int:
    """Lane groups of a full MSV grid (MSV_HMM.describe()): the kernel's n_groups, its statically assigned
    first indices."""
    return info["blocks"] * info["waves_per_block"] * 64 // info["lanes_per_group"]


def msv_capacity(info: dict, name: str) -> int:
    """Sequences a full MSV grid holds at once: D streams per lane group."""
    return msv_groups(info) * msv_streams(name)


def take_sequences(codes: np.ndarray, offsets: np.ndarray, idx: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """The CSR batch of sequences idx[0], idx[1], ... (vectorised gather)."""
    idx = np.asarray(idx, np.int64)
    off = offsets.astype(np.int64)
    lens = (off[1:] - off[:-1])[idx]
    out_off = np.zeros(len(idx) + 1, np.int64)
    np.cumsum(lens, out=out_off[1:])
    total = int(out_off[-1])
    if total == 0:
        return np.zeros(0, np.uint8), out_off.astype(np.uint64)
    # residue j of output sequence k comes from off[idx[k]] + j: one shift per sequence, repeated over its residues
    src = np.repeat(off[idx] - out_off[:-1], lens) + np.arange(total, dtype=np.int64)
    return np.ascontiguousarray(codes[src]), out_off.astype(np.uint64)


def prefix(codes: np.ndarray, offsets: np.ndarray, n: int) -> tuple[np.ndarray, np.ndarray]:
    """The first n sequences of a CSR batch (views)."""
    return codes[:int(offsets[n])], offsets[:n + 1]


def queue_batch(match_emissions: np.ndarray, seed: int, n: int, lmax: int = 130) -> tuple[np.ndarray, np.ndarray]:
    """A CSR batch of exactly n sequences for a queue deeper than the grid: uniform random sequences of
    length U[1, lmax] (the bulk, vectorised), ~1,500 sequences emitted by the profile's match states and ~1,500
    emitted along gapped paths (length U[lmax / 2, lmax]), and 40 copies of each edge length (0, 1, 2, 3, 63, 64,
    65, 127, 128, 129) -- all shuffled by a seeded permutation, so every kind lands throughout the queue."""
    n_edge = EDGE_COPIES * len(EDGE_LENGTHS)
    n_hom = min(HOMOLOGS, n // 8)
    n_bulk = n - n_edge - 2 * n_hom
    if n_bulk < 0:
        raise ValueError(f"queue_batch needs n >= {n_edge * 4 // 3 + 1}")
    rng = np.random.Generator(np.random.PCG64(seed))
    edge_lens = np.repeat(np.array(EDGE_LENGTHS, np.uint64), EDGE_COPIES)
    edge_off = np.zeros(n_edge + 1, np.uint64)
    np.cumsum(edge_lens, out=edge_off[1:])
    edge = (rng.integers(0, 20, int(edge_off[-1]), dtype=np.uint8), edge_off)
    hmin = max(1, lmax // 2)
    codes, offsets = concat_batches(random_batch(seed + 1, n_bulk, 1, lmax),
                                    homolog_batch(match_emissions, seed + 2, n_hom, hmin, lmax),
                                    gapped_homolog_batch(match_emissions, seed + 3, n_hom, hmin, lmax), edge)
    assert len(offsets) - 1 == n
    return take_sequences(codes, offsets, rng.permutation(n))
