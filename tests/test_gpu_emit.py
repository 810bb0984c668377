"""The emit stage on the GPU (emit.hip, emit_device.cpp; msv.h "Emit stage").

The three launches of msv_emit_batch_device are compared byte for byte with msv_emit_generate, THE definition: codes,
offsets, domain offsets, domains, ops and truncated flags, into buffers of exactly the totals with a guard band behind
each, at n around the wave (64, the walk kernels' workgroup), its multiples and the scan's 1024 runs, for a first
above 2^32, with and without flanks, unihit and multihit, both insert modes, on synthetic models of LENG 1 .. 65 and
the bundled 100.hmm and 2405.hmm.  A capacity one short returns the error with every byte untouched; truncated walks
equal the definition; the call shapes (no truth, chunked workspaces, a second stream, two emitters interleaved) give
the same bytes; and the device batch goes into the three engines' device calls with no host copy, their scores equal
bit for bit to score_batch on the downloaded bytes."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import hmm_fasta_viterbi_amd as msv
from hmm_fasta_viterbi_amd import _native
from hmm_fasta_viterbi_amd.synthetic import write_hmm

from emit_lib import DATA

BLOCK = 64  # emitk::kWalkBlock
NS = [1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025]
FIRSTS = [0, (1 << 32) + 987654321]
CONFIGS = [(0, True, msv.INSERTS_ZERO), (1, False, msv.INSERTS_LOG_ODDS), (400, True, msv.INSERTS_ZERO),
           (400, False, msv.INSERTS_LOG_ODDS), (1, True, msv.INSERTS_LOG_ODDS), (0, False, msv.INSERTS_ZERO)]
GUARD = 64
OUT_OF_MEMORY = "MSV_ERR_OUT_OF_MEMORY"


def _torch():
    import torch
    return torch


def _profile(tmp_path, name):
    if isinstance(name, int):
        path = os.path.join(str(tmp_path), f"synthetic_{name}.hmm")
        write_hmm(path, name, 1000 + name)
        return msv.Profile_HMM(path)
    return msv.Profile_HMM(f"{DATA}/{name}.hmm")


class Buffers:
    """Device buffers of exactly the given sizes, each with a guard band of a fill pattern behind it."""

    def __init__(self, n, residues, domains, ops, short=None):
        torch = _torch()
        dev = torch.device("cuda:0")
        self.n = n
        self.cap = {"codes": residues, "domains": domains, "ops": ops}
        if short:
            self.cap[short] -= 1
        self.sizes = {"codes": self.cap["codes"], "offsets": 8 * (n + 1), "domain_offsets": 8 * (n + 1),
                      "domains": 32 * self.cap["domains"], "ops": self.cap["ops"], "truncated": n}
        self.t = {k: torch.full((v + GUARD,), 0xEE, dtype=torch.uint8, device=dev) for k, v in self.sizes.items()}
        for v in self.t.values():
            assert v.data_ptr() % 16 == 0

    def truth(self):
        return _native.EmitTruth(self.t["domain_offsets"].data_ptr(), self.t["domains"].data_ptr(),
                                 self.cap["domains"], self.t["ops"].data_ptr(), self.cap["ops"],
                                 self.t["truncated"].data_ptr())

    def host(self):
        return {k: v.cpu().numpy() for k, v in self.t.items()}

    def guards_intact(self, host, untouched=()):
        ok = True
        for k, a in host.items():
            ok &= bool(np.all(a[self.sizes[k]:] == 0xEE))
            if k in untouched:
                ok &= bool(np.all(a == 0xEE))
        return ok


def device_emit(emitter, want, n, seed, first, truth=True, stream=None):
    """msv_emit_batch_device into exact guarded buffers -> the downloaded bytes as the definition's tuple."""
    torch = _torch()
    codes, off, doff, doms, ops, trunc = want
    b = Buffers(n, len(codes), len(doms), len(ops))
    st = stream or torch.cuda.Stream(torch.device("cuda:0"))
    torch.cuda.synchronize()
    tot = emitter.emit_into(n, b.t["codes"].data_ptr(), b.cap["codes"], b.t["offsets"].data_ptr(), seed=seed,
                            first=first, truth=b.truth() if truth else None, stream=st.cuda_stream)
    h = b.host()
    assert b.guards_intact(h, () if truth else ("domain_offsets", "domains", "ops", "truncated"))
    assert tot["residues"] == len(codes) and tot["overflow"] == 0 and tot["truncated"] == int(trunc.sum())
    assert tot["domains"] == len(doms) and tot["ops"] == len(ops)
    got = [h["codes"][:len(codes)], h["offsets"][:8 * (n + 1)].view(np.uint64)]
    if truth:
        got += [h["domain_offsets"][:8 * (n + 1)].view(np.uint64),
                h["domains"][:32 * len(doms)].view(_native.DOMAIN_DTYPE), h["ops"][:len(ops)],
                h["truncated"][:n].astype(bool)]
    return got


def assert_equal(got, want, what):
    names = ("codes", "offsets", "domain_offsets", "domains", "ops", "truncated")
    for name, g, w in zip(names, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, w.dtype, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), (what, name)


@pytest.mark.parametrize("name", [1, 2, 3, 63, 64, 65, "100"])
def test_bytes_equal_the_definition(tmp_path, name):
    profile = _profile(tmp_path, name)
    calls = 0
    for Lc, multihit, insert_mode in CONFIGS:
        e = msv.Emitter(profile, length=Lc, multihit=multihit, insert_mode=insert_mode)
        for first in FIRSTS:
            whole = msv.emit_generate(profile, max(NS), 42, first, length=Lc, multihit=multihit,
                                      insert_mode=insert_mode)
            for n in NS:
                # the definition of the first n sequences is the slice of the larger call (tests/test_emit_paths.py)
                want = msv.emit_generate(profile, n, 42, first, length=Lc, multihit=multihit,
                                         insert_mode=insert_mode) if n < 200 else _head(whole, n)
                assert_equal(device_emit(e, want, n, 42, first), want, (name, Lc, multihit, insert_mode, first, n))
                calls += 1
        e.close()
    print(f"emit bytes {name}: {calls} device calls equal the definition")


def _head(whole, n):
    codes, off, doff, doms, ops, trunc = whole
    d = doms[:int(doff[n])]
    o = int(d["ops_begin"][-1] + d["ops_len"][-1]) if len(d) else 0
    return codes[:int(off[n])], off[:n + 1], doff[:n + 1], d, ops[:o], trunc[:n]


def test_a_few_thousand_and_2405(tmp_path):
    profile = _profile(tmp_path, "100")
    e = msv.Emitter(profile)
    want = msv.emit_generate(profile, 5000, 7)
    assert_equal(device_emit(e, want, 5000, 7, 0), want, "100.hmm n = 5000")
    print(f"emit bytes 100.hmm: n = 5000, {len(want[0])} residues, {len(want[3])} domains")
    big = _profile(tmp_path, "2405")
    for Lc, multihit, insert_mode in ((400, True, msv.INSERTS_ZERO), (0, False, msv.INSERTS_LOG_ODDS)):
        e = msv.Emitter(big, length=Lc, multihit=multihit, insert_mode=insert_mode)
        for first in FIRSTS:
            want = msv.emit_generate(big, 64, 42, first, length=Lc, multihit=multihit, insert_mode=insert_mode)
            assert_equal(device_emit(e, want, 64, 42, first), want, ("2405.hmm", Lc, first))
        print(f"emit bytes 2405.hmm Lc {Lc}: n = 64, {len(want[0])} residues, {len(want[4])} ops")


@pytest.mark.parametrize("short", ["codes", "domains", "ops"])
def test_capacity_one_short_writes_nothing(tmp_path, short):
    torch = _torch()
    profile = _profile(tmp_path, "100")
    e = msv.Emitter(profile, length=20)
    n = 300
    codes, off, doff, doms, ops, trunc = msv.emit_generate(profile, n, 42, length=20)
    b = Buffers(n, len(codes), len(doms), len(ops), short=short)
    st = torch.cuda.Stream(torch.device("cuda:0"))
    torch.cuda.synchronize()
    with pytest.raises(msv.MSVError) as err:
        e.emit_into(n, b.t["codes"].data_ptr(), b.cap["codes"], b.t["offsets"].data_ptr(), seed=42, truth=b.truth(),
                    stream=st.cuda_stream)
    print(f"emit capacity one {short} short: {err.value.name}, totals {err.value.totals}")
    assert err.value.name == OUT_OF_MEMORY
    assert err.value.totals["overflow"] == {"codes": 1, "domains": 2, "ops": 4}[short]
    assert err.value.totals["residues"] == len(codes)
    assert b.guards_intact(b.host(), untouched=tuple(b.sizes))
    # the same handle then serves a call that fits
    want = (codes, off, doff, doms, ops, trunc)
    assert_equal(device_emit(e, want, n, 42, 0), want, "after an overflow")


@pytest.mark.parametrize("cut", [1, 2, 17])
def test_truncation_equals_the_definition(tmp_path, cut):
    profile = _profile(tmp_path, "100")
    for Lc in (0, 400):
        e = msv.Emitter(profile, length=Lc, max_length=cut)
        want = msv.emit_generate(profile, 200, 9, length=Lc, max_length=cut)
        assert want[5].any()
        assert_equal(device_emit(e, want, 200, 9, 0), want, ("cut", cut, Lc))
        print(f"emit truncation at {cut}, Lc {Lc}: {int(want[5].sum())} of 200 truncated, equal")


def test_call_shapes(tmp_path):
    torch = _torch()
    profile = _profile(tmp_path, "100")
    e = msv.Emitter(profile, length=60)
    n = 700
    want = msv.emit_generate(profile, n, 42, length=60)
    # no truth: the same codes and offsets, and no truth buffer is touched
    got = device_emit(e, want, n, 42, 0, truth=False)
    assert_equal(got, want[:2], "truth = NULL")
    r = e.emit(n, truth=False)
    assert r.traces is None and r.codes.tobytes() == want[0].tobytes() and r.offsets.tobytes() == want[1].tobytes()
    # the host call: one chunk at exactly its workspace, more below it, the same bytes
    need = msv.Emitter.workspace_bytes(n, len(want[0]), len(want[3]), len(want[4]))
    for ws, chunks in ((0, 1), (need, 1), (need - 1, None), (need // 5, None), (4096, None)):
        r = e.emit(n, workspace_bytes=ws, scores=False)
        print(f"emit workspace {ws}: {r.chunks} chunks")
        assert r.chunks == chunks if chunks else r.chunks > 1
        assert_equal((r.codes, r.offsets, r.traces.domain_offsets, r.traces.domains, r.traces.ops, r.truncated),
                     want, ("workspace", ws))
    with pytest.raises(msv.MSVError) as err:
        e.emit(n, workspace_bytes=64)
    assert err.value.name == OUT_OF_MEMORY
    # a second stream, a bound stream, and the scores of the traces
    st = torch.cuda.Stream(torch.device("cuda:0"))
    assert_equal(device_emit(e, want, n, 42, 0, stream=st), want, "a second stream")
    e.bind_stream(st.cuda_stream)
    r = e.emit(n)
    e.bind_stream(None)
    assert r.codes.tobytes() == want[0].tobytes()
    assert np.array_equal(r.traces.scores, e.cpu_emit(n).traces.scores)
    # two emitters on two streams, interleaved
    e2 = msv.Emitter(profile, length=5, multihit=False)
    want2 = msv.emit_generate(profile, n, 43, length=5, multihit=False)
    s1, s2 = torch.cuda.Stream(torch.device("cuda:0")), torch.cuda.Stream(torch.device("cuda:0"))
    for _ in range(3):
        assert_equal(device_emit(e, want, n, 42, 0, stream=s1), want, "emitter 1")
        assert_equal(device_emit(e2, want2, n, 43, 0, stream=s2), want2, "emitter 2")
    # n = 0 and the arguments
    tot = e.emit_into(0, None, 0, torch.zeros(1, dtype=torch.int64, device="cuda:0").data_ptr(), stream=st.cuda_stream)
    assert tot["residues"] == 0 and tot["overflow"] == 0
    with pytest.raises(msv.MSVError):
        e.emit_into(1, None, 0, None, stream=st.cuda_stream)
    with pytest.raises(msv.MSVError):
        e.emit_into(1, None, 0, torch.zeros(2, dtype=torch.int64, device="cuda:0").data_ptr(), stream=None)


@pytest.mark.parametrize("name", ["100", "1400"])
def test_chaining_into_the_engines(tmp_path, name):
    """The device batch goes straight into the engines' device calls: no host copy of residues or offsets."""
    torch = _torch()
    profile = _profile(tmp_path, name)
    e = msv.Emitter(profile, length=100)
    n = 257
    st = torch.cuda.Stream(torch.device("cuda:0"))
    batch = e.emit_device(n, seed=5, stream=st.cuda_stream)
    codes = batch["codes"].cpu().numpy()[:batch["residues_len"]]
    offsets = batch["offsets"].cpu().numpy().view(np.uint64)
    want = msv.emit_generate(profile, n, 5, length=100)
    assert codes.tobytes() == want[0].tobytes() and offsets.tobytes() == want[1].tobytes()
    longest = int(np.diff(offsets).max())
    for engine in (msv.MSV_HMM(profile), msv.Viterbi_HMM(profile), msv.Forward_HMM(profile)):
        engine.reserve_length(longest)
        d_sc = torch.full((n,), 7.0, dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        engine.score_batch_device(batch["codes_ptr"], batch["residues_len"], batch["offsets_ptr"], n, d_sc.data_ptr(),
                                  stream=st.cuda_stream)
        engine.check(st.cuda_stream)
        got = d_sc.cpu().numpy()
        host = engine.score_batch(codes=codes, offsets=offsets)
        same = np.array_equal(got.view(np.uint32), host.view(np.uint32))
        print(f"emit chaining {name}.hmm {type(engine).__name__}: {n} scores, bit-identical {same}, "
              f"mean {float(got.mean()):.2f} nats")
        assert same and np.all(np.isfinite(got))
        engine.close()


def test_resources(tmp_path):
    info = msv.Emitter(_profile(tmp_path, "2405")).describe()
    print(f"emit describe: {info}")
    assert info["count_scratch_bytes"] == 0 and info["place_scratch_bytes"] == 0 and info["scan_scratch_bytes"] == 0
    assert info["block"] == BLOCK and info["count_vgprs"] > 0 and info["place_vgprs"] > 0
    assert info["table_bytes"] < 400 * 1024 and info["model_length"] == 2406
