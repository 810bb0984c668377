"""The bias filter on the GPU (bias_filter.hip) against the library's float64 twin (msv_bf_cpu_score).

The bound is msv.h's ("Bias filter"), derived from the kernel's roundings, not measured: |gpu - cpu| <= k u / (1 - k u)
+ u |cpu| with k = 5 L + 14 ceil(L / 1024) + 4.  The lengths sit on the edges of a lane's chunk (16) and of a trip
(1,024).  A bias is a function of the sequence and the profile alone, so placement, select list and stream are
compared bitwise.  The filtered selection and the cascade are compared with the host arithmetic (msv_bf_pvalues) on
the DEVICE's own scores and bias, so no decision is compared across float32 / float64.  The worst error / bound
ratio is printed before it is asserted; DESIGN 4.13 records it."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import hmm_fasta_viterbi_amd as msv
from hmm_fasta_viterbi_amd import _native

import bias_filter_lib as bfl
from bias_filter_lib import EXPONENTIAL, GUMBEL, LENGTHS, pvalues, tolerance
from oracle_lib import ROOT, bits, profile_path
from state_batches import _csr

MODELS = bfl.models()


@pytest.fixture(scope="module")
def engines():
    out = {name: msv.Bias_filter(m) for name, m in MODELS.items()}
    yield out
    for e in out.values():
        e.close()


def to_device(codes, offsets):
    import torch
    dev = torch.device("cuda:0")
    c = codes if codes.size else np.zeros(1, np.uint8)
    return torch.from_numpy(c).to(dev), torch.from_numpy(offsets.view(np.int64)).to(dev)


def device_scores(e, codes, offsets, select=None, count=None, stream=None, fill=7.0):
    """msv_bf_score_batch_device on a fresh copy of the batch -> float32 [n] (entries not written keep `fill`)."""
    import torch
    n = len(offsets) - 1
    d_res, d_off = to_device(codes, offsets)
    assert d_res.data_ptr() % 16 == 0
    d_out = torch.full((n,), fill, dtype=torch.float32, device=d_res.device)
    d_sel = d_cnt = None
    if select is not None:
        d_sel = torch.from_numpy(np.ascontiguousarray(select, np.uint32).view(np.int32)).to(d_res.device)
        d_cnt = torch.tensor([len(select) if count is None else count], dtype=torch.int32, device=d_res.device)
    st = stream if stream is not None else torch.cuda.Stream(d_res.device)
    torch.cuda.synchronize()
    e.score_batch_device(d_res.data_ptr(), codes.size, d_off.data_ptr(), n, d_out.data_ptr(),
                         d_sel.data_ptr() if d_sel is not None else None,
                         d_cnt.data_ptr() if d_cnt is not None else None, st.cuda_stream)
    st.synchronize()
    return d_out.cpu().numpy(), st


def test_describe(engines):
    d = engines["100"].describe()
    assert d["residues_per_lane"] == bfl.CHUNK and d["residues_per_trip"] == bfl.TRIP
    assert d["scratch_bytes"] == 0 and d["model_length"] == 101 and d["blocks"] >= 1
    compo, bg, M = MODELS["100"]
    table = np.zeros(26, np.float32)
    assert _native.lib().msv_bf_device_table(compo.ctypes.data, bg.ctypes.data, M, table.ctypes.data) == 0
    assert np.array_equal(np.array(d["table"], np.float32).view(np.uint32), table.view(np.uint32))


# ---- lengths ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(MODELS))
def test_every_length_edge_within_the_derived_tolerance(engines, name):
    compo, bg, M = MODELS[name]
    e = engines[name]
    worst = 0.0
    for kind, (codes, offsets) in bfl.length_batches(compo, bg, seed=M).items():
        assert list(np.diff(offsets)) == LENGTHS
        got = e.score_batch(codes=codes, offsets=offsets)
        st, want = bfl.cpu_score_batch(compo, bg, M, codes, offsets)
        assert st == 0 and got.dtype == np.float32 and np.all(np.isfinite(got))
        assert got[0] == 0.0 and want[0] == 0.0
        tol = tolerance(np.diff(offsets), want)
        ratio = np.abs(got.astype(np.float64) - want) / tol
        print(f"bias filter {name} {kind}: worst error / bound {ratio.max():.4f} at L = {LENGTHS[int(ratio.argmax())]}; "
              f"bias {want.min():.3f} .. {want.max():.3f}")
        worst = max(worst, float(ratio.max()))
        assert np.all(ratio <= 1.0), (name, kind, ratio)
        # the host call and the device call are one kernel
        dev, _ = device_scores(e, codes, offsets)
        assert np.array_equal(bits(dev), bits(got))
    print(f"bias filter {name}: worst error / bound {worst:.4f}")


# ---- placement --------------------------------------------------------------------------------------------------------

def test_a_bias_does_not_depend_on_alignment_select_list_or_stream(engines):
    import torch
    e = engines["100"]
    rng = np.random.Generator(np.random.PCG64(5))
    x = rng.integers(0, 20, 1025).astype(np.uint8)
    seqs, where = [], []
    pos = 0
    for a in range(16):  # x at every byte alignment: a filler brings the offset to a (mod 16)
        filler = (a - pos) % 16
        seqs.append(rng.integers(0, 20, filler).astype(np.uint8))
        pos += filler
        assert pos % 16 == a
        where.append(len(seqs))
        seqs.append(x)
        pos += len(x)
    seqs.append(rng.integers(0, 20, 5000).astype(np.uint8))  # and behind a long one
    where.append(len(seqs))
    seqs.append(x)
    codes, offsets = _csr(seqs)
    assert sorted(int(offsets[w]) % 16 for w in where[:16]) == list(range(16))
    got, _ = device_scores(e, codes, offsets)
    assert len(where) == 17 and len(set(bits(got[where]).tolist())) == 1
    alone = e.score_batch(codes=x, offsets=np.array([0, 1025], np.uint64))
    assert bits(alone)[0] == bits(got[where])[0]
    # a select list in another order, and a second stream
    n = len(offsets) - 1
    sel = rng.permutation(n).astype(np.uint32)
    listed, _ = device_scores(e, codes, offsets, select=sel)
    assert np.array_equal(bits(listed), bits(got))
    other, _ = device_scores(e, codes, offsets, stream=torch.cuda.Stream(torch.device("cuda:0")))
    assert np.array_equal(bits(other), bits(got))
    e.check()


# ---- lists ------------------------------------------------------------------------------------------------------------

def _small_batch(seed=9):
    rng = np.random.Generator(np.random.PCG64(seed))
    return _csr([rng.integers(0, 20, L).astype(np.uint8) for L in (30, 0, 1025, 17, 400, 1024)])


def test_an_empty_select_list_leaves_the_buffer_untouched(engines):
    codes, offsets = _small_batch()
    got, st = device_scores(engines["100"], codes, offsets, select=np.array([2, 3], np.uint32), count=0)
    assert np.all(got == np.float32(7.0))
    engines["100"].check(st.cuda_stream)


def test_a_select_entry_outside_the_batch_is_latched_and_its_neighbours_scored(engines):
    e = engines["100"]
    codes, offsets = _small_batch()
    n = len(offsets) - 1
    want = e.score_batch(codes=codes, offsets=offsets)
    got, st = device_scores(e, codes, offsets, select=np.array([4, n, 0, n + 7, 2], np.uint32))
    for s in (4, 0, 2):
        assert bits(got)[s] == bits(want)[s]
    assert got[1] == np.float32(7.0) and got[3] == np.float32(7.0) and got[5] == np.float32(7.0)
    with pytest.raises(msv.MSVError) as err:
        e.check(st.cuda_stream)
    assert err.value.name == "MSV_ERR_INVALID_ARGUMENT"
    e.check(st.cuda_stream)  # reported once, then cleared


def test_a_bad_code_gives_inf_there_and_an_index_error(engines):
    e = engines["100"]
    codes, offsets = _small_batch()
    want = e.score_batch(codes=codes, offsets=offsets)
    bad = codes.copy()
    bad[int(offsets[3]) - 1] = 20  # the last residue of the 1,025-long sequence
    got, st = device_scores(e, bad, offsets)
    assert got[2] == np.inf
    keep = [0, 1, 3, 4, 5]
    assert np.array_equal(bits(got[keep]), bits(want[keep]))
    with pytest.raises(IndexError):
        e.check(st.cuda_stream)
    e.check(st.cuda_stream)
    with pytest.raises(IndexError):
        e.score_batch(codes=bad, offsets=offsets)
    assert np.array_equal(bits(e.score_batch(codes=codes, offsets=offsets)), bits(want))  # (its own bits only)


# ---- the cascade's engines and batch ----------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def cascade():
    h = msv.Profile_HMM(profile_path("100"))
    eng = {"hmm": h, "msv": msv.MSV_HMM(h), "vit": msv.Viterbi_HMM(h), "fwd": msv.Forward_HMM(h),
           "bias": msv.Bias_filter(h)}
    codes, offsets = bfl.cascade_batch()
    eng["codes"], eng["offsets"] = codes, offsets
    eng["msv_scores"] = eng["msv"].score_batch(codes=codes, offsets=offsets)
    eng["bias_all"] = eng["bias"].score_batch(codes=codes, offsets=offsets)
    yield eng
    for k in ("msv", "vit", "fwd", "bias"):
        eng[k].close()


# ---- select -----------------------------------------------------------------------------------------------------------

def _select(fn, scores, bias, offsets, order, mu, lam, threshold):
    """msv_bf_filter_select_device (bias given) or msv_filter_select_device -> (list, P-values)."""
    import torch
    n = len(scores)
    dev = torch.device("cuda:0")
    d_sc = torch.from_numpy(scores).to(dev)
    d_off = torch.from_numpy(offsets.view(np.int64)).to(dev)
    d_ord = torch.from_numpy(order.view(np.int32)).to(dev) if order is not None else None
    d_pv = torch.full((n,), -1.0, dtype=torch.float64, device=dev)
    d_sel = torch.full((n,), -1, dtype=torch.int32, device=dev)
    d_cnt = torch.full((1,), -1, dtype=torch.int32, device=dev)
    st = torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    args = [0, d_sc.data_ptr()]
    if bias is not None:
        d_b = torch.from_numpy(bias).to(dev)
        torch.cuda.synchronize()
        args.append(d_b.data_ptr())
    args += [d_off.data_ptr(), d_ord.data_ptr() if d_ord is not None else None, n, mu, lam, threshold,
             d_pv.data_ptr(), d_sel.data_ptr(), d_cnt.data_ptr(), st.cuda_stream]
    assert getattr(_native.lib(), fn)(*args) == 0
    st.synchronize()
    cnt = int(d_cnt.cpu().numpy()[0])
    assert 0 <= cnt <= n
    return d_sel.cpu().numpy()[:cnt].astype(np.int64), d_pv.cpu().numpy()


@pytest.mark.parametrize("threshold", [0.02, 0.3])
@pytest.mark.parametrize("ordered", [False, True])
def test_filtered_selection_is_the_host_decision_in_order(cascade, threshold, ordered):
    sc, b, offsets = cascade["msv_scores"], cascade["bias_all"], cascade["offsets"]
    n = len(sc)
    h = cascade["hmm"]
    mu, lam = h.stats_local_msv_mu, h.stats_local_msv_lambda
    order = np.random.Generator(np.random.PCG64(4)).permutation(n).astype(np.uint32) if ordered else None
    walk = order.astype(np.int64) if ordered else np.arange(n)
    got, pv = _select("msv_bf_filter_select_device", sc, b, offsets, order, mu, lam, threshold)
    st, want_pv = pvalues(sc, b, offsets, mu, lam, GUMBEL)
    assert st == 0
    assert np.array_equal(got, walk[want_pv[walk] <= threshold])
    assert np.array_equal(pv.view(np.uint64), want_pv.view(np.uint64)) or np.allclose(pv, want_pv, rtol=1e-12, atol=0)
    assert 0 < len(got) < n
    # with a zero bias the list is msv_filter_select_device's
    zero = np.zeros(n, np.float32)
    a, pa = _select("msv_bf_filter_select_device", sc, zero, offsets, order, mu, lam, threshold)
    c, pc = _select("msv_filter_select_device", sc, None, offsets, order, mu, lam, threshold)
    assert np.array_equal(a, c) and np.array_equal(pa.view(np.uint64), pc.view(np.uint64))
    assert len(got) < len(c)  # the filter removes the planted sequences


def test_filtered_forward_pvalues_on_the_device(cascade):
    import torch
    sc, b, offsets = cascade["msv_scores"], cascade["bias_all"], cascade["offsets"]
    n = len(sc)
    dev = torch.device("cuda:0")
    d_sc, d_b = torch.from_numpy(sc).to(dev), torch.from_numpy(b).to(dev)
    d_off = torch.from_numpy(offsets.view(np.int64)).to(dev)
    for kind, loc in ((GUMBEL, -8.5), (EXPONENTIAL, -3.0)):
        d_pv = torch.full((n,), -1.0, dtype=torch.float64, device=dev)
        st = torch.cuda.Stream(dev)
        torch.cuda.synchronize()
        assert _native.lib().msv_bf_pvalues_device(0, d_sc.data_ptr(), d_b.data_ptr(), d_off.data_ptr(), n, loc, 0.7,
                                                   kind, d_pv.data_ptr(), st.cuda_stream) == 0
        st.synchronize()
        s, want = pvalues(sc, b, offsets, loc, 0.7, kind)
        assert s == 0 and np.allclose(d_pv.cpu().numpy(), want, rtol=1e-12, atol=0)


# ---- cascade ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("F1,F2", [(0.02, 1e-3), (0.5, 0.5)])
def test_cascade_with_the_bias_filter(cascade, F1, F2):
    h = cascade["hmm"]
    codes, offsets = cascade["codes"], cascade["offsets"]
    n = len(offsets) - 1
    out = msv.search_pipeline(cascade["msv"], cascade["vit"], cascade["fwd"], codes=codes, offsets=offsets, F1=F1,
                              F2=F2, bias_engine=cascade["bias"])
    A, B, Cm = out["passed_msv"], out["passed_bias"], out["passed_vit"]
    bias = out["bias"]
    assert np.all(A[B]) and np.all(B[Cm]) and np.all(bias[~A] == 0.0)
    # every stage's scores are that stage's own engine's, bitwise
    assert np.array_equal(bits(out["msv_scores"]), bits(cascade["msv_scores"]))
    assert np.array_equal(bits(bias[A]), bits(cascade["bias_all"][A]))
    vit_all = cascade["vit"].score_batch(codes=codes, offsets=offsets)
    fwd_all = cascade["fwd"].score_batch(codes=codes, offsets=offsets)
    assert np.array_equal(bits(out["vit_scores"][B]), bits(vit_all[B])) and np.all(out["vit_scores"][~B] == -np.inf)
    assert np.array_equal(bits(out["fwd_scores"][Cm]), bits(fwd_all[Cm])) and np.all(out["fwd_scores"][~Cm] == -np.inf)
    # every mask and every P-value is the host arithmetic on the device's scores and bias
    zero = np.zeros(n, np.float32)
    p1 = pvalues(out["msv_scores"], zero, offsets, h.stats_local_msv_mu, h.stats_local_msv_lambda, GUMBEL)[1]
    p1f = pvalues(out["msv_scores"], bias, offsets, h.stats_local_msv_mu, h.stats_local_msv_lambda, GUMBEL)[1]
    p2f = pvalues(out["vit_scores"], bias, offsets, h.stats_local_viterbi_mu, h.stats_local_viterbi_lambda, GUMBEL)[1]
    p3f = pvalues(out["fwd_scores"], bias, offsets, h.stats_local_forward_theta, h.stats_local_forward_lambda,
                  EXPONENTIAL)[1]
    assert np.array_equal(A, p1 <= F1)
    assert np.array_equal(B, p1f <= F1)
    assert np.array_equal(Cm, p2f <= F2)
    assert np.array_equal(out["fwd_pvalues"], p3f)
    assert np.all(p1f[~A] == p1[~A])  # a zero bias reproduces the null1 P-value
    if F1 == 0.02:
        # the planted sequence the CPU premise names (tests/test_bias_filter_host.py) is out, by the filter alone
        _, _, bits1, bits2, cut = bfl.cascade_reference()
        planted = np.arange(bfl.N_BACKGROUND, n)
        removed = planted[(bits1[planted] >= cut + 1.0) & (bits2[planted] <= cut - 1.0)]
        assert removed.size >= 1 and np.all(A[removed]) and not np.any(B[removed]) and not np.any(Cm[removed])
    print(f"cascade F1 {F1} F2 {F2}: MSV {int(A.sum())}, bias filter {int(B.sum())}, Viterbi {int(Cm.sum())} of {n}")
    assert int(B.sum()) < int(A.sum())


def test_cascade_without_a_bias_engine_is_unchanged(cascade):
    codes, offsets = cascade["codes"], cascade["offsets"]
    lib = _native.lib()
    a = msv.search_pipeline(cascade["msv"], cascade["vit"], cascade["fwd"], codes=codes, offsets=offsets)
    b = msv.search_pipeline(cascade["msv"], cascade["vit"], cascade["fwd"], codes=codes, offsets=offsets,
                            bias_engine=None)
    assert list(a) == ["msv_scores", "passed_msv", "vit_scores", "passed_vit", "fwd_scores", "fwd_pvalues"]
    assert list(a) == list(b)
    # ... and the options entry with the flag off is msv_fwd_filter_batch, output for output
    n = len(offsets) - 1
    h = cascade["hmm"]
    stats = np.array([h.stats_local_msv_mu, h.stats_local_msv_lambda, h.stats_local_viterbi_mu,
                      h.stats_local_viterbi_lambda, h.stats_local_forward_theta, h.stats_local_forward_lambda],
                     np.float32)
    msc, vsc, fsc = (np.zeros(n, np.float32) for _ in range(3))
    p1, p2, pb = (np.zeros(n, np.uint8) for _ in range(3))
    fpv, bias = np.zeros(n), np.full(n, 5.0, np.float32)
    n1, n2, nb = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    opt = _native.SearchOptions(C.sizeof(_native.SearchOptions), 0, 0, None)
    assert lib.msv_fwd_filter_batch_opts(
        cascade["msv"]._p, cascade["vit"]._p, cascade["fwd"]._p, codes.ctypes.data, offsets.ctypes.data, n,
        stats.ctypes.data, 0.02, 1e-3, C.byref(opt), msc.ctypes.data, p1.ctypes.data, vsc.ctypes.data, p2.ctypes.data,
        fsc.ctypes.data, fpv.ctypes.data, C.byref(n1), C.byref(n2), bias.ctypes.data, pb.ctypes.data,
        C.byref(nb)) == 0
    got = {"msv_scores": msc, "passed_msv": p1.astype(bool), "vit_scores": vsc, "passed_vit": p2.astype(bool),
           "fwd_scores": fsc, "fwd_pvalues": fpv}
    for k in a:
        assert a[k].dtype == b[k].dtype == got[k].dtype
        assert a[k].tobytes() == b[k].tobytes() == got[k].tobytes(), k
    assert np.all(bias == 0.0) and np.array_equal(pb, p1) and nb.value == n1.value == int(p1.sum())
    # the flag without a profile is refused
    opt = _native.SearchOptions(C.sizeof(_native.SearchOptions), 1, 0, None)
    assert lib.msv_fwd_filter_batch_opts(
        cascade["msv"]._p, cascade["vit"]._p, cascade["fwd"]._p, codes.ctypes.data, offsets.ctypes.data, n,
        stats.ctypes.data, 0.02, 1e-3, C.byref(opt), msc.ctypes.data, p1.ctypes.data, vsc.ctypes.data, p2.ctypes.data,
        fsc.ctypes.data, fpv.ctypes.data, C.byref(n1), C.byref(n2), bias.ctypes.data, pb.ctypes.data,
        C.byref(nb)) == 1


def test_msv_filter_and_filter_pipeline_with_the_bias_filter(cascade):
    codes, offsets = cascade["codes"], cascade["offsets"]
    h = cascade["hmm"]
    out = msv.search_pipeline(cascade["msv"], cascade["vit"], cascade["fwd"], codes=codes, offsets=offsets,
                              bias_engine=cascade["bias"])
    sc, fpv, mask, b = cascade["msv"].msv_filter(codes=codes, offsets=offsets, bias=cascade["bias"])
    assert np.array_equal(mask, out["passed_bias"]) and np.array_equal(bits(b), bits(out["bias"]))
    assert np.array_equal(fpv, cascade["bias"].pvalues(sc, b, offsets, kind="msv"))
    msc, passed, vsc, vpv, b2 = msv.filter_pipeline(cascade["msv"], cascade["vit"], codes=codes, offsets=offsets,
                                                    bias_engine=cascade["bias"])
    assert np.array_equal(passed, out["passed_bias"]) and np.array_equal(bits(vsc), bits(out["vit_scores"]))
    assert np.array_equal(bits(b2), bits(out["bias"])) and np.array_equal(bits(msc), bits(out["msv_scores"]))
    want = pvalues(vsc, b2, offsets, h.stats_local_viterbi_mu, h.stats_local_viterbi_lambda, GUMBEL)[1]
    assert np.array_equal(vpv[passed], want[passed]) and np.all(np.isnan(vpv[~passed]))
    # defaults: the calls without the argument return what they returned before it existed
    plain = cascade["msv"].msv_filter(codes=codes, offsets=offsets)
    assert len(plain) == 3 and np.array_equal(plain[2], out["passed_msv"])
    assert len(msv.filter_pipeline(cascade["msv"], cascade["vit"], codes=codes, offsets=offsets)) == 4


# ---- the C++ surface ----------------------------------------------------------------------------------------------------

def test_cpp_bias_filter_driver():
    exe = os.path.join(_native.LIB_DIR, "test_bias_filter")
    p = subprocess.run([exe, ROOT], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "test_bias_filter passed" in p.stdout, p.stdout + p.stderr
