"""Residue positions in the upper half of the 32-bit range, BITWISE.

The device entry points accept residues_len < 2^32 and the MSV kernels keep residue positions as uint32_t
(st.pos, st.endpos, st.endp and the block prefetch indices pos + lane + 16, msv_kernel_body.inc); the largest
offset any other test reaches is ~4 * 10^8.  Here one zero-filled device buffer of 2^32 - 1 bytes holds a small
batch twice -- straddling 2^31, and ending exactly at byte 2^32 - 1, where pos + lane wraps and the last
sequence's end equals the 0xFFFFFFFF that marks a retired stream -- and every plan scores both placements
exactly as at offset 0 and as the oracle.  Every address a lane can form lies inside the buffer (the kernels
clamp each index to the sequence's last residue; the Viterbi kernels index 64-bit, relative to the sequence's
start, and so need no residues_len bound).  residues_len = 2^32 is refused, and the host entry points rebase
64-bit offsets above 2^32."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import hmm_fasta_viterbi_amd as msv
from hmm_fasta_viterbi_amd.synthetic import concat_batches, homolog_batch, random_batch
from oracle_lib import OracleProfile, bits, profile_path
from queue_batches import take_sequences
from state_batches import edge_batch, tail_homolog_batch

BUF = (1 << 32) - 1  # bytes: the largest residues_len the device entry points accept
_buf = {}


def big_buffer():
    """The zero-filled device buffer, allocated once for the module."""
    import torch
    if "d" not in _buf:
        _buf["d"] = torch.zeros(BUF, dtype=torch.uint8, device="cuda:0")
    return _buf["d"]


def teardown_module(module):
    _buf.clear()
    import torch
    torch.cuda.empty_cache()


def mixed_batch(prof, n):
    """n sequences of lengths 0..130: tail homologs (paths through the last states), homologs, uniform ones and
    the edge lengths, shuffled; the batch's last sequence is not empty (so it ends where the placement says)."""
    me = msv.Profile_HMM(profile_path(prof)).match_emissions
    seed = int(prof.split(".")[0])
    k = max(8, n // 8)
    codes, offsets = concat_batches(tail_homolog_batch(me, seed, k, 1, 130), homolog_batch(me, seed + 1, k, 1, 130),
                                    edge_batch(seed + 2), random_batch(seed + 3, n - 2 * k - 6, 0, 130))
    rng = np.random.Generator(np.random.PCG64(seed + 4))
    perm = rng.permutation(n)
    lens = np.diff(offsets.astype(np.int64))
    last = int(np.nonzero(lens[perm] > 0)[0][-1])
    perm[[last, n - 1]] = perm[[n - 1, last]]
    return take_sequences(codes, offsets, perm)


def placements(total):
    """Byte offset of the batch's first residue: at 0, straddling 2^31, ending exactly at byte 2^32 - 1."""
    return {"zero": 0, "straddles_2^31": (1 << 31) - total // 2, "ends_at_2^32-1": BUF - total}


class DeviceBatch:
    """A CSR batch placed at `base` in the big buffer (absolute 64-bit offsets on the device)."""

    def __init__(self, codes, offsets, base):
        import torch
        self.buf = big_buffer()
        self.n = len(offsets) - 1
        self.base, self.total = base, int(offsets[-1])
        assert 0 <= base and base + self.total <= BUF
        self.buf[base:base + self.total] = torch.from_numpy(codes).to(self.buf.device)
        self.off = torch.from_numpy((offsets.astype(np.uint64) + np.uint64(base)).view(np.int64)).to(self.buf.device)
        self.order = torch.empty(max(self.n, 1), dtype=torch.int32, device=self.buf.device)
        self.st = torch.cuda.Stream(self.buf.device)
        torch.cuda.synchronize()

    def clear(self):
        import torch
        self.buf[self.base:self.base + self.total] = 0
        torch.cuda.synchronize()

    def msv(self, e, n, longest_first):
        import torch
        sc = torch.full((n,), 7.0, dtype=torch.float32, device=self.buf.device)
        torch.cuda.synchronize()
        if longest_first:
            e.order_longest_first(self.off.data_ptr(), n, self.order.data_ptr(), self.st.cuda_stream)
        e.score_batch_device(self.buf.data_ptr(), BUF, self.off.data_ptr(), n, sc.data_ptr(),
                             self.order.data_ptr() if longest_first else None, self.st.cuda_stream)
        self.st.synchronize()
        e.check(self.st.cuda_stream)
        return sc.cpu().numpy()

    def vit(self, v, n):
        import torch
        sc = torch.full((n,), 7.0, dtype=torch.float32, device=self.buf.device)
        torch.cuda.synchronize()
        v.score_batch_device(self.buf.data_ptr(), BUF, self.off.data_ptr(), n, sc.data_ptr(), None, None,
                             self.st.cuda_stream)
        self.st.synchronize()
        v.check(self.st.cuda_stream)
        return sc.cpu().numpy()


@pytest.mark.parametrize("prof,main", [("100.hmm", "msv_g4_"), ("1400.hmm", "msv_g16_"), ("2405.hmm", "_a")],
                         ids=["100_narrow", "1400_blocks", "2405_split"])
def test_msv_device_batches_at_high_offsets(prof, main):
    """msv_score_batch_device with residues_len = 2^32 - 1 on 100.hmm (narrow whole-row plan), 1400.hmm (16-lane
    residue blocks) and 2405.hmm (split): batch sizes that take the cooperative plan, the plan after it (latency,
    or the 16-lane plan of 100.hmm) and -- forced, so that a few hundred sequences reach it -- the throughput
    plan, with d_order NULL and longest first."""
    e = msv.MSV_HMM(msv.Profile_HMM(profile_path(prof)))
    f = msv.MSV_HMM(msv.Profile_HMM(profile_path(prof)))
    try:
        info = e.describe()
        assert main in info["variant"] and info["coop_max_n"] >= 64, info
        f.set_variant(info["variant"])
        n_all = int(info["coop_max_n"]) + 200
        codes, offsets = mixed_batch(prof, n_all)
        want = OracleProfile(prof).score_batch(codes, offsets, threads=8)
        sizes = [(e, 1), (e, 60), (e, int(info["coop_max_n"]) + 1), (e, n_all), (f, n_all)]
        plans = [x.variant_for(n) for x, n in sizes]
        assert plans[0] == plans[1] == info["coop_variant"] and plans[2] != info["coop_variant"]
        assert plans[4] == info["variant"], plans
        for where, base in placements(int(offsets[-1])).items():
            d = DeviceBatch(codes, offsets, base)
            for (x, n), plan in zip(sizes, plans):
                for longest_first in (False, True):
                    got = d.msv(x, n, longest_first)
                    assert np.array_equal(bits(got), bits(want[:n])), (prof, where, plan, n, longest_first,
                                                                       np.nonzero(bits(got) != bits(want[:n]))[0][:8])
            d.clear()
        print(f"{prof}: plans {plans} at offsets {placements(int(offsets[-1]))}")
    finally:
        e.close()
        f.close()


@pytest.mark.parametrize("prof,waves", [("400.hmm", 1), ("1400.hmm", 1), ("2405.hmm", 2)])
def test_viterbi_device_batches_at_high_offsets(prof, waves):
    """msv_vit_score_batch_device on the same placements: the single-wave kernel (400.hmm), the one-wave team
    (1400.hmm) and the two-wave team (2405.hmm)."""
    v = msv.Viterbi_HMM(msv.Profile_HMM(profile_path(prof)))
    try:
        info = v.describe()
        assert info["waves_per_sequence"] == waves and info["variant"].startswith("vit_w") == (prof != "400.hmm"), info
        codes, offsets = mixed_batch(prof, 300)
        want = OracleProfile(prof).vit_score_batch(codes, offsets, threads=8)
        for where, base in placements(int(offsets[-1])).items():
            d = DeviceBatch(codes, offsets, base)
            got = d.vit(v, 300)
            assert np.array_equal(bits(got), bits(want)), (prof, where, info["variant"])
            d.clear()
    finally:
        v.close()


def test_residues_len_of_2_to_32_is_refused():
    """residues_len = 2^32 returns MSV_ERR_INVALID_ARGUMENT from msv_score_batch_device and
    msv_score_grid_device and launches nothing: the scores keep their fill and no error is latched."""
    import torch
    dev = torch.device("cuda:0")
    engines = [msv.MSV_HMM(msv.Profile_HMM(profile_path(p))) for p in ("100.hmm", "1400.hmm")]
    try:
        codes, offsets = random_batch(3, 20, 1, 50)
        r = torch.from_numpy(codes).to(dev)
        o = torch.from_numpy(offsets.view(np.int64)).to(dev)
        s = torch.full((2, 20), 7.0, dtype=torch.float32, device=dev)
        st = torch.cuda.Stream(dev)
        torch.cuda.synchronize()
        for call in (lambda: engines[0].score_batch_device(r.data_ptr(), 1 << 32, o.data_ptr(), 20, s.data_ptr(), None,
                                                           st.cuda_stream),
                     lambda: msv.score_grid_device(engines, r.data_ptr(), 1 << 32, o.data_ptr(), 20, s.data_ptr(), None,
                                                   st.cuda_stream)):
            with pytest.raises(msv.MSVError) as err:
                call()
            assert err.value.name == "MSV_ERR_INVALID_ARGUMENT"
        st.synchronize()
        for e in engines:
            e.check(st.cuda_stream)
        assert bool((s == 7.0).all())
        # the largest accepted length right below it still scores
        engines[0].score_batch_device(r.data_ptr(), r.numel(), o.data_ptr(), 20, s.data_ptr(), None, st.cuda_stream)
        engines[0].check(st.cuda_stream)
        assert np.array_equal(bits(s[0].cpu().numpy()), bits(OracleProfile("100").score_batch(codes, offsets)))
    finally:
        for e in engines:
            e.close()


def test_host_calls_rebase_offsets_above_2_to_32():
    """msv_score_batch and msv_vit_score_batch with a host pointer and 64-bit offsets[0] above 2^32: a lazily
    allocated zero buffer of which only the pages under the batch are touched."""
    prof = "1400.hmm"
    codes, offsets = mixed_batch(prof, 300)
    base = (1 << 32) + 123457
    host = np.zeros(base + int(offsets[-1]), np.uint8)
    host[base:] = codes
    off = offsets.astype(np.uint64) + np.uint64(base)
    o = OracleProfile(prof)
    h = msv.Profile_HMM(profile_path(prof))
    e, v = msv.MSV_HMM(h), msv.Viterbi_HMM(h)
    try:
        assert np.array_equal(bits(e.score_batch(codes=host, offsets=off)), bits(o.score_batch(codes, offsets)))
        assert np.array_equal(bits(e.score_batch(codes=host, offsets=off[:41])), bits(o.score_batch(codes, offsets))[:40])
        assert np.array_equal(bits(v.score_batch(codes=host, offsets=off)), bits(o.vit_score_batch(codes, offsets)))
    finally:
        e.close()
        v.close()
