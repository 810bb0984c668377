"""The Forward kernel (fwd_kernel.hip) at every variant's lane edges and scan steps, on batches aimed there.

The stage is held to a tolerance, not to bits, and the tolerance is loose: an error has to move a score by more than
it to be seen.  tests/forward_batches.py builds models and sequences whose scores hang on one thing each -- a D
chain that only scan step j can deliver, the last state, the first, a transition across a lane boundary, an I state
in a lane's last or first slot -- with every transition distinct per node, and tests/test_forward_batches.py shows
on the CPU that each moves its sequences by hundreds to tens of thousands of tolerances.  Here every variant runs
them: at LENG 64 S, 64 S - S + 1 (one real state in the last lane) and 64 S - S (the last lane all padding), with
zeros inside the scan, and with a queue deeper than the grid.

Every comparison is forward_lib.assert_close against cpu_scores (the library's float64 Forward) on the same tables,
with msv.h's tolerance: |gpu - cpu64| <= 16 (L + LENG) 2^-24 + 4 2^-24 |cpu64| nats, -inf / finite classes equal.
DESIGN 4.9 records the worst error per test as assert_close prints it."""
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import hmm_fasta_viterbi_amd as msv
from hmm_fasta_viterbi_amd import _native
from hmm_fasta_viterbi_amd.synthetic import concat_batches, random_batch
from forward_batches import (DD, aimed_batch, base_model, bridge_model, bridge_sequences, insertion_batch, knocked,
                             queue_batch, rescaled_chain, with_transition)
from forward_lib import assert_close, cpu_scores, create_profile, destroy_profile, gpu_scores, tolerance
from oracle_lib import bits
from queue_batches import take_sequences
from state_batches import _csr, interleave

VARIANTS = ["fwd_s2", "fwd_s6", "fwd_s12", "fwd_s22g", "fwd_s38g4",
            "fwd_s2i", "fwd_s6i", "fwd_s12i", "fwd_s22gi", "fwd_s38g4i"]


def shape_of(name):
    """(S, insert odds) of a variant name."""
    return int(re.match(r"fwd_s(\d+)", name).group(1)), name.endswith("i")


def test_parametrisation_is_every_variant():
    assert VARIANTS == msv.Forward_HMM.variants()


class Profile:
    """A raw device profile over a model's tables, forced to one variant; describe() is checked on entry."""

    def __init__(self, model, name):
        self.model, self.name = model, name

    def __enter__(self):
        S, isc = shape_of(self.name)
        assert (self.model[1] is not None) == isc
        self.p = create_profile(*self.model, self.name)
        info = _native.FwdInfo()
        assert _native.lib().msv_fwd_profile_describe(self.p, info) == 0
        self.info = info.as_dict()
        assert self.info["variant"] == self.name and self.info["states_per_lane"] == S, self.info
        assert self.info["scratch_bytes"] == 0 and self.info["model_length"] == self.model[0].shape[1], self.info
        return self

    def __exit__(self, *exc):
        destroy_profile(self.p)

    def host(self, codes, offsets):
        st, got = gpu_scores(self.p, codes, offsets)
        assert st == 0, _native.STATUS.get(st, st)
        return got

    def device(self, codes, offsets):
        """One launch over a device-resident batch in queue order (no select list) on a stream of its own."""
        import torch
        dev = torch.device("cuda:0")
        n = len(offsets) - 1
        d_res = torch.from_numpy(np.ascontiguousarray(codes)).to(dev)
        d_off = torch.from_numpy(np.ascontiguousarray(offsets, np.uint64).view(np.int64)).to(dev)
        d_sc = torch.full((n,), 7.0, dtype=torch.float32, device=dev)
        stream = torch.cuda.Stream(dev)
        torch.cuda.synchronize()
        st = _native.lib().msv_fwd_score_batch_device(self.p, d_res.data_ptr(), codes.size, d_off.data_ptr(), n, None,
                                                      None, d_sc.data_ptr(), stream.cuda_stream)
        assert st == 0, _native.STATUS.get(st, st)
        stream.synchronize()
        assert _native.lib().msv_fwd_profile_check(self.p, stream.cuda_stream) == 0
        return d_sc.cpu().numpy()


def edge_batch_of(model, S):
    (aimed, where), (ins, _) = aimed_batch(model, S, 32), insertion_batch(model, S, 42)
    return concat_batches(aimed, ins), where


# ---- capacity edges -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", VARIANTS)
def test_capacity_edges(name):
    """LENG 64 S, 64 S - S + 1 and 64 S - S: tail homologs ending in state LENG, head homologs starting in state 1,
    windows across the lane boundaries 0|1, 15|16, 31|32, 62|63 and the last real lane's, the edge lengths, and
    insertions in a lane's last and first slot; the insert-odds variants on an informative insert table.  Once
    through the host call, once as a device launch in queue order (same bits)."""
    S, isc = shape_of(name)
    for short, leng in enumerate((64 * S, 64 * S - S + 1, 64 * S - S)):
        model = base_model(leng, 31 + short, isc)
        (codes, offsets), where = edge_batch_of(model, S)
        assert len(where["tail"]) == 24 and len(where["head"]) == 24 and len(where["window"]) >= 4
        assert len(offsets) - 1 <= 150 and int(np.diff(offsets.astype(np.int64)).max()) <= 130
        want = cpu_scores(*model, codes, offsets)
        with Profile(model, name) as p:
            got = p.host(codes, offsets)
            assert_close(got, want, offsets, leng, f"capacity edges {name} LENG {leng}, host call")
            dev = p.device(codes, offsets)
            assert_close(dev, want, offsets, leng, f"capacity edges {name} LENG {leng}, device launch")
            assert np.array_equal(bits(dev), bits(got))


# ---- bridges: the scan, step by step -------------------------------------------------------------------------------

def bridge_plain(model, S):
    """The six bridge sequences at flanks of 0, 1 and 3 residues, and the other source / landing pairings."""
    return concat_batches(*[bridge_sequences(model, S, 70 + f, flank=f) for f in (0, 1, 3)],
                          bridge_sequences(model, S, 75, cross=True))


def bridge_batches(model, S):
    """(bridge_plain's sequences between uniform ones, their indices), and the same with a rescaled chain of 12 hits
    in front of every bridge sequence."""
    plain = bridge_plain(model, S)
    n = len(plain[1]) - 1
    fill = random_batch(74, n, 1, 130)
    seqs = [plain[0][int(plain[1][i]):int(plain[1][i + 1])] for i in range(n)]
    chained = _csr([np.concatenate([rescaled_chain(model, 80 + i), s]) for i, s in enumerate(seqs)])
    (a, wa), (b, wb) = interleave({"bridge": plain}, fill), interleave({"bridge": chained}, fill)
    return (a, wa["bridge"]), (b, wb["bridge"])


@pytest.mark.parametrize("name", VARIANTS)
def test_bridges(name):
    """bridge_model at LENG 64 S: the score of bridge j's sequence hangs on a D chain that crosses more than 2^j
    lane boundaries between a source in a lane's first or last slot and its landing, with d->d, m->d and d->m
    distinct at every node -- a scan multiplier A[j] taken for another lane, a c_q off by a slot or a shifted *_IN
    array moves it by thousands of tolerances (test_forward_batches.py).  Then the same behind a chain of 12 hits,
    so that the scale's exponent is not 0 where the bridge is crossed."""
    S, isc = shape_of(name)
    model = bridge_model(S, 11, isc)
    (plain, at_plain), (chained, at_chained) = bridge_batches(model, S)
    with Profile(model, name) as p:
        for what, (codes, offsets), at in (("bridges", plain, at_plain),
                                           ("bridges behind a chain", chained, at_chained)):
            want = cpu_scores(*model, codes, offsets)
            if what != "bridges":
                assert want[at].min() > 5 * 22.2, want[at]  # several crossings of 2^32 before the bridge
            got = p.host(codes, offsets)
            assert_close(got, want, offsets, 64 * S, f"{what} {name}")
            assert_close(got[at], want[at], np.concatenate([[0], np.cumsum(np.diff(offsets.astype(np.int64))[at])]),
                         64 * S, f"{what} {name}, the bridge sequences alone")


# ---- zeros inside the scan -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", VARIANTS)
def test_zeros_in_the_scan(name):
    """An odds of exactly 0 inside the model: a node closed (match column, d->d, m->d, d->m at -inf) in a lane's last
    slot (lane 31), in a lane's first slot (lane 32) and in lane 0 -- every A[j] and c_q across it is exactly 0 and
    the D chain restarts behind it; d->d at -inf at every node (every A[j] is 0); and d->d at 0, odds 1, at every
    node (every A[j] and c_q is 1: the chain is a plain prefix sum).  GPU and CPU on the same tables, with the
    bridge sequences (two bridges cross lane 31 | 32), the windows, tails, heads and edge lengths."""
    S, isc = shape_of(name)
    leng = 64 * S
    model = bridge_model(S, 11, isc)
    codes, offsets = concat_batches(bridge_plain(model, S), aimed_batch(model, S, 33)[0])
    assert len(offsets) - 1 <= 150
    cases = {"node 32 S closed": knocked(model, 32 * S), "node 32 S + 1 closed": knocked(model, 32 * S + 1),
             "node 2 closed": knocked(model, 2), "d->d -inf everywhere": with_transition(model, DD, -np.inf),
             "d->d 0 everywhere": with_transition(model, DD, 0.0)}
    intact = cpu_scores(*model, codes, offsets)
    for what, zeroed in cases.items():
        want = cpu_scores(*zeroed, codes, offsets)
        with np.errstate(invalid="ignore"):
            felt = np.abs(want - intact) / tolerance(np.diff(offsets.astype(np.int64)), leng, intact)
        assert np.nanmax(felt) > 100.0, what  # the zeros carry weight
        with Profile(zeroed, name) as p:
            assert_close(p.host(codes, offsets), want, offsets, leng, f"{what}, {name}")


# ---- queue depth ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", VARIANTS)
def test_every_wave_of_every_variant_scores_several_sequences(name):
    """2 x blocks x waves_per_block + 3 sequences at LENG 64 S -- homologs and uniform sequences of length 0 .. 24 and
    one rescaled chain of 80 residues in every 64, shuffled: every wave takes several sequences, so an exponent, N, J,
    C or a row register that survived from the previous sequence shows (4 waves per workgroup and their exit count
    at S = 38, the fenced rows from S = 22 on)."""
    S, isc = shape_of(name)
    leng = 64 * S
    model = base_model(leng, 91, isc)
    with Profile(model, name) as p:
        n = 2 * p.info["blocks"] * p.info["waves_per_block"] + 3
        (codes, offsets), chains = queue_batch(model, n, 92)
        lens = np.diff(offsets.astype(np.int64))
        assert len(lens) == n and lens[chains].tolist() == [80] * len(chains) and np.delete(lens, chains).max() <= 24
        want = cpu_scores(*model, codes, offsets)
        assert want[chains].min() > 2 * 22.2 + 3.0, want[chains].min()  # E has passed 2^32 (22.2 nats) more than once
        got = p.host(codes, offsets)
        assert_close(got, want, offsets, leng, f"queue depth {name}, n = {n}")
        again = p.host(codes, offsets)  # the counters were reset by the last workgroup to leave
        assert np.array_equal(bits(again), bits(got))


# ---- determinism ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", VARIANTS[:5])
def test_aimed_batch_permuted_gives_the_same_bits(name):
    S, isc = shape_of(name)
    model = base_model(64 * S, 31, isc)
    (codes, offsets), _ = edge_batch_of(model, S)
    n = len(offsets) - 1
    perm = np.random.Generator(np.random.PCG64(95)).permutation(n)
    pc, po = take_sequences(codes, offsets, perm)
    with Profile(model, name) as p:
        a = p.host(codes, offsets)
        b = p.host(pc, po)
    assert np.array_equal(bits(b), bits(a[perm]))
