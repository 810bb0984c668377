"""The lazy-E rows of the long whole-row MSV variants (msv_kernel_body.inc, LAZY), BITWISE against the oracle.

A row of these kernels skips its E maximum when a per-lane bound proves that no lane of the wave can raise its
group's J; the skip is wave-uniform, so the four sequences of a wave decide it together.  The batches here make
lean and full rows alternate inside a wave: uniform-random sequences (J a slowly decaying record: mostly lean
rows), sequences emitted by the profile (J records and J >= N: full rows), one residue repeated, a hit in the
last rows, the shortest lengths (J = -inf: the first rows are never lean), and residue codes >= 20 at the first,
a middle and the last position (the poison row is never lean: +inf and the error bit as before).  Two profiles:
1400.hmm on the plan the benchmark runs, forced, and 1100.hmm, whose 16 x 72 plan leaves its last lane mostly
padding (a bound of -inf in most residue rows).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import hmm_fasta_viterbi_amd as msv
from hmm_fasta_viterbi_amd.synthetic import homolog_batch, random_batch
from oracle_lib import OracleProfile, bits, profile_path
from queue_batches import msv_capacity, queue_batch

CASES = [("1400.hmm", "msv_g16_s88_w16_p2_d1"), ("1100.hmm", "msv_g16_s72_w16_p2_d1")]
_state = {}


def csr(seqs):
    off = np.zeros(len(seqs) + 1, np.uint64)
    np.cumsum([len(s) for s in seqs], out=off[1:])
    return (np.concatenate(seqs).astype(np.uint8) if off[-1] else np.zeros(0, np.uint8)), off


def sequences(codes, offsets):
    return [codes[int(offsets[i]):int(offsets[i + 1])] for i in range(len(offsets) - 1)]


def mixed_batch(hmm, seed):
    """176 sequences, shuffled so every wave of four holds several kinds."""
    rng = np.random.Generator(np.random.PCG64(seed))
    me = hmm.match_emissions
    seqs = []
    for length in (0, 1, 2, 3, 17):  # the shortest: J = -inf on the first rows
        seqs += [rng.integers(0, 20, length, dtype=np.uint8) for _ in range(4)]
    seqs += sequences(*random_batch(seed + 1, 60, 300, 500))
    seqs += sequences(*random_batch(seed + 2, 24, 20, 120))
    hom = sequences(*homolog_batch(me, seed + 3, 40, 300, 500))  # J records, J >= N
    seqs += hom
    seqs += [np.full(n, r, np.uint8) for r, n in ((0, 400), (7, 333), (19, 64), (12, 5))]  # one residue repeated
    # the best hit in the last rows: random residues, then the tail of a profile-emitted sequence
    for k in range(8):
        tail = hom[k][-(30 + 10 * k):]
        seqs.append(np.concatenate([rng.integers(0, 20, 300 + 7 * k, dtype=np.uint8), tail]))
    # ... and one whose single strong row is the last one
    seqs.append(np.concatenate([rng.integers(0, 20, 349, dtype=np.uint8), hom[9][-1:]]))
    # a hit, a long random stretch (J decays: lean rows), a second hit (full rows again)
    for k in range(8):
        seqs.append(np.concatenate([hom[10 + k][:80], rng.integers(0, 20, 250, dtype=np.uint8), hom[20 + k][:60]]))
    # the rest: random again, so the count is a multiple of the wave's four
    seqs += sequences(*random_batch(seed + 4, 176 - len(seqs), 300, 500))
    order = rng.permutation(len(seqs))
    return csr([seqs[i] for i in order])


def case(prof, name):
    if prof not in _state:
        hmm = msv.Profile_HMM(profile_path(prof))
        e = msv.MSV_HMM(hmm)
        e.set_variant(name)
        assert e.describe()["variant"] == name and e.variant_for(176) == name
        codes, offsets = mixed_batch(hmm, 900 + int(prof.split(".")[0]))
        assert 64 <= len(offsets) - 1 <= 300
        want = OracleProfile(prof).score_batch(codes, offsets)
        _state[prof] = dict(hmm=hmm, e=e, codes=codes, offsets=offsets, want=want)
    return _state[prof]


def same(got, want):
    g, w = bits(got), bits(want)
    if np.array_equal(g, w):
        return True
    bad = np.nonzero(g != w)[0]
    print(f"{len(bad)} of {len(g)} scores differ, first at {bad[:12].tolist()}: got {np.asarray(got)[bad[:6]]} "
          f"want {np.asarray(want)[bad[:6]]}")
    return False


def device_scores(e, codes, offsets):
    """One device launch in queue order; returns (scores, stream) with the error word still latched."""
    import torch
    dev = torch.device("cuda:0")
    n = len(offsets) - 1
    r = torch.from_numpy(np.ascontiguousarray(codes)).to(dev)
    o = torch.from_numpy(np.ascontiguousarray(offsets).view(np.int64)).to(dev)
    s = torch.full((n,), 7.0, dtype=torch.float32, device=dev)
    st = torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    e.score_batch_device(r.data_ptr(), r.numel(), o.data_ptr(), n, s.data_ptr(), None, st.cuda_stream)
    st.synchronize()
    return s.cpu().numpy(), st


@pytest.mark.parametrize("prof,name", CASES)
def test_mixed_batch_bitwise(prof, name):
    """The mixed batch through the host call (longest first: similar sequences share a wave) and as one device
    launch in queue order (the shuffled kinds share a wave)."""
    g = case(prof, name)
    assert same(g["e"].score_batch(codes=g["codes"], offsets=g["offsets"]), g["want"]), (prof, "host call")
    got, st = device_scores(g["e"], g["codes"], g["offsets"])
    g["e"].check(st.cuda_stream)
    assert same(got, g["want"]), (prof, "device launch")


@pytest.mark.parametrize("prof,name", CASES)
def test_mixed_batch_zero_copy_twin(prof, name):
    """The same batch with its residues in page-locked host memory: the plan's zero-copy twin."""
    g = case(prof, name)
    pc = msv.pinned_empty(g["codes"].size, np.uint8)
    pc[:] = g["codes"]
    assert same(g["e"].score_batch(codes=pc, offsets=g["offsets"]), g["want"]), prof


@pytest.mark.parametrize("prof,name", CASES)
def test_poison_residue_is_never_skipped(prof, name):
    """A code >= 20 at the first, a middle and the last position of a 300-500-residue sequence (and alone in a
    1-residue one), late in sequences whose rows were lean before it: +inf exactly there, the error reported
    once, every other score of the launch bitwise."""
    g = case(prof, name)
    seqs = [s.copy() for s in sequences(g["codes"], g["offsets"])]
    long_ones = [i for i, s in enumerate(seqs) if 300 <= len(s) <= 500][:3]
    one = next(i for i, s in enumerate(seqs) if len(s) == 1)
    for i, pos, code in zip(long_ones, (0, len(seqs[long_ones[1]]) // 2, len(seqs[long_ones[2]]) - 1), (20, 25, 255)):
        seqs[i][pos] = code
    seqs[one][0] = 21
    planted = long_ones + [one]
    codes, offsets = csr(seqs)
    got, st = device_scores(g["e"], codes, offsets)
    with pytest.raises(IndexError):
        g["e"].check(st.cuda_stream)
    g["e"].check(st.cuda_stream)  # reported once, then clean
    assert np.all(np.isposinf(got[planted])), got[planted]
    rest = np.ones(len(seqs), bool)
    rest[planted] = False
    assert same(got[rest], g["want"][rest]), prof
    with pytest.raises(IndexError):  # the host call reports it too
        g["e"].score_batch(codes=codes, offsets=offsets)
    assert same(g["e"].score_batch(codes=g["codes"], offsets=g["offsets"]), g["want"]), (prof, "clean call after")


def test_queue_three_rounds_deep():
    """3 * capacity + 17 short sequences in one launch on the benchmark's plan: every lane group restarts its
    stream (bound and J reset per lane) while the other three groups of its wave are in mid-sequence."""
    prof, name = CASES[0]
    g = case(prof, name)
    capacity = msv_capacity(g["e"].describe(), name)
    n = 3 * capacity + 17
    codes, offsets = queue_batch(g["hmm"].match_emissions, 9100, n, lmax=48)
    want = OracleProfile(prof).score_batch(codes, offsets, threads=16)
    got, st = device_scores(g["e"], codes, offsets)
    g["e"].check(st.cuda_stream)
    assert same(got, want), (prof, capacity, n)


def test_unequal_e_transitions_keep_every_row_full():
    """tr_E_C != tr_E_J: C is no longer J, so no row may skip its E.  A profile over 1400.hmm's tables with
    tr_E_C lowered, forced onto the benchmark's plan, against the float32 restatement of the recurrence on
    the first 64 sequences of the mixed batch."""
    import ctypes as C
    from hmm_fasta_viterbi_amd import _native
    from state_batches import numpy_msv
    prof, name = CASES[0]
    g = case(prof, name)
    L = _native.lib()
    es, tBM, tEC, tEJ = g["hmm"].msv_scores()
    es = np.ascontiguousarray(es, np.float32)
    tEC2 = float(np.float32(tEC) - np.float32(0.75))
    n = 64
    offsets = np.ascontiguousarray(g["offsets"][:n + 1])
    codes = np.ascontiguousarray(g["codes"][:int(offsets[n])])
    want = numpy_msv(es, tBM, tEC2, tEJ, codes, offsets)
    p = C.c_void_p()
    assert L.msv_profile_create(0, es.ctypes.data, es.shape[1], tBM, tEC2, tEJ, C.byref(p)) == 0
    try:
        assert L.msv_profile_set_variant(p, name.encode()) == 0
        got = np.zeros(n, np.float32)
        assert L.msv_score_batch(p, codes.ctypes.data, offsets.ctypes.data, n, got.ctypes.data, None) == 0
    finally:
        L.msv_profile_destroy(p)
    assert same(got, want)
