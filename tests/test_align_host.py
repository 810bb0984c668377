"""The alignment stage's host-only layer (aln_host.cpp; msv.h "Alignment stage") on bundled profiles:
the float64 decode against decode_lib.np_decode's full matrices in log space, the row sums, the three special terms
against occ, the envelope score against the CPU Forward and under another configured length, the workspace and chunk
arithmetic, and the argument errors."""
import ctypes as C
import os

import numpy as np
import pytest

import hmm_fasta_viterbi_amd as msv
from hmm_fasta_viterbi_amd import _native
from hmm_fasta_viterbi_amd.synthetic import homolog_batch
import align_lib
import decode_lib
import forward_lib
from forward_batches import base_model, consensus

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILES = (("100.hmm", 0), ("100.hmm", 1), ("200.hmm", 0))


def _model(prof, mode):
    return forward_lib.tables(msv.Profile_HMM(os.path.join(ROOT, "data", "profile_HMMs", prof)), mode)


def np_posteriors(model, codes):
    """ppM, ppI of msv.h from decode_lib.np_decode's recurrences restated with the matrices kept (log space)."""
    msc, isc, tsc, consts = model
    from forward_lib import MM, MI, MD, IM, II, DM, DD
    tBM, tEC, tEJ = (float(x) for x in consts)
    M = msc.shape[1]
    K, L = M - 1, len(codes)
    loop, move = (float(x) for x in msv.sequence_transitions(L))
    la, NI = np.logaddexp, -np.inf
    m = msc.astype(np.float64)
    ins = np.zeros((20, M)) if isc is None else isc.astype(np.float64)
    t = np.full((M + 1, 7), NI)
    t[1:K] = tsc[1:K].astype(np.float64)
    with np.errstate(invalid="ignore"):
        fM, fI, fD = (np.full((L + 1, M + 2), NI) for _ in range(3))
        fN, fJ, fC, fB = (np.full(L + 1, NI) for _ in range(4))
        fN[0], fB[0] = 0.0, move
        for i in range(1, L + 1):
            r = codes[i - 1]
            prev = la(la(fM[i - 1, 0:K] + t[0:K, MM], fI[i - 1, 0:K] + t[0:K, IM]), fD[i - 1, 0:K] + t[0:K, DM])
            fM[i, 1:K + 1] = m[r, 1:K + 1] + la(prev, fB[i - 1] + tBM)
            fI[i, 1:K] = ins[r, 1:K] + la(fM[i - 1, 1:K] + t[1:K, MI], fI[i - 1, 1:K] + t[1:K, II])
            for k in range(2, K + 1):
                fD[i, k] = la(fM[i, k - 1] + t[k - 1, MD], fD[i, k - 1] + t[k - 1, DD])
            E = la(np.logaddexp.reduce(fM[i, 1:K + 1]), np.logaddexp.reduce(fD[i, 2:K + 1]) if K >= 2 else NI)
            fN[i] = fN[i - 1] + loop
            fJ[i] = la(fJ[i - 1] + loop, E + tEJ)
            fC[i] = la(fC[i - 1] + loop, E + tEC)
            fB[i] = la(fN[i], fJ[i]) + move
        Z = fC[L] + move
        bM, bI, bD = (np.full((L + 2, M + 2), NI) for _ in range(3))
        bJ, bC, bN = (np.full(L + 2, NI) for _ in range(3))
        bC[L] = move
        bE = tEC + bC[L]
        for k in range(K, 0, -1):
            bD[L, k] = la(bE if k >= 2 else NI, t[k, DD] + bD[L, k + 1])
            bM[L, k] = la(bE, t[k, MD] + bD[L, k + 1])
        for i in range(L - 1, 0, -1):
            r = codes[i]
            bB = tBM + np.logaddexp.reduce(m[r, 1:K + 1] + bM[i + 1, 1:K + 1])
            bJ[i] = la(loop + bJ[i + 1], move + bB)
            bC[i] = loop + bC[i + 1]
            bN[i] = la(loop + bN[i + 1], move + bB)
            bE = la(tEJ + bJ[i], tEC + bC[i])
            for k in range(K, 0, -1):
                g = m[r, k + 1] + bM[i + 1, k + 1] if k < K else NI
                h = ins[r, k] + bI[i + 1, k] if k < K else NI
                bD[i, k] = la(la(bE if k >= 2 else NI, t[k, DM] + g), t[k, DD] + bD[i, k + 1])
                bM[i, k] = la(la(la(bE, t[k, MM] + g), t[k, MI] + h), t[k, MD] + bD[i, k + 1])
                bI[i, k] = la(t[k, IM] + g, t[k, II] + h)
        ppM = np.exp(fM[1:L + 1, :M] + bM[1:L + 1, :M] - Z)
        ppI = np.exp(fI[1:L + 1, :M] + bI[1:L + 1, :M] - Z)
    return ppM, ppI


@pytest.fixture(scope="module", params=PROFILES, ids=lambda p: f"{p[0]}-{p[1]}")
def decoded(request):
    prof, mode = request.param
    model = _model(prof, mode)
    hmm = msv.Profile_HMM(os.path.join(ROOT, "data", "profile_HMMs", prof))
    codes, offsets = homolog_batch(hmm.match_emissions, 7, 2, 30, 45)
    seqs = [codes[int(offsets[i]):int(offsets[i + 1])] for i in range(2)]
    return model, [(c, align_lib.cpu_decode(model, c), decode_lib.np_decode(*model, c), np_posteriors(model, c))
                   for c in seqs]


def test_posteriors_are_the_log_space_matrices(decoded):
    model, runs = decoded
    for codes, (st, score, pm, pi, pn, pj, pc), ref, (wm, wi) in runs:
        assert st == 0 and abs(score - ref["fwd"]) <= 1e-9 * abs(score)
        assert np.max(np.abs(pm - wm)) <= 1e-9 and np.max(np.abs(pi - wi)) <= 1e-9
        assert pm.sum() > 0.3 * len(codes)  # homologs: a good part of the mass is on the match states
        assert np.all(pm[:, 0] == 0) and np.all(pi[:, 0] == 0) and np.all(pi[:, -1] == 0)


def test_rows_sum_to_one_and_the_specials_are_what_occ_leaves(decoded):
    model, runs = decoded
    for codes, (st, score, pm, pi, pn, pj, pc), ref, _ in runs:
        rows = pm.sum(axis=1) + pi.sum(axis=1) + pn + pj + pc
        assert np.max(np.abs(rows - 1.0)) <= 1e-9
        assert np.max(np.abs(pn + pj + pc - (1.0 - ref["occ"]))) <= 1e-9
        assert np.max(np.abs(pm.sum(axis=1) + pi.sum(axis=1) - ref["occ_core"])) <= 1e-9


def test_whole_sequence_score_is_the_cpu_forward(decoded):
    model, runs = decoded
    for codes, (st, score, *_), _, _ in runs:
        st, want = forward_lib.cpu_score(*model, codes)
        assert st == 0 and score == want


def test_configured_length_moves_the_score_as_loop_and_move_predict():
    """A flank-free consensus item: every path with weight emits all Le residues in one domain, none in N, J or C,
    so Z carries move twice (N -> B, C -> T) and no loop: the score moves by 2 (move(Lc) - move(Le))."""
    msc, isc, tsc, consts = base_model(40, 5, True)
    best = np.argmax(msc[:, 1:], axis=0)
    msc[:, 1:] = np.float32(np.log(20.0 * 0.001 / 19.0))  # every node one residue at 0.999: nothing pays for a flank
    msc[best, np.arange(1, 41)] = np.float32(np.log(20.0 * 0.999))
    model = (msc, isc, tsc, consts)
    codes = consensus(model, 1, 40)
    st, s0, pm, pi, pn, pj, pc = align_lib.cpu_decode(model, codes)
    flank0 = float((pn + pj + pc).sum())  # the share of Z on paths that emit any residue outside the core
    # (a local model never is flank-free to the last digit: skipping an end residue costs one match emission)
    assert st == 0 and flank0 < 0.2
    for Lc in (400, 5000):
        st, s1, *post = align_lib.cpu_decode(model, codes, Lc)
        assert st == 0
        predicted = 2.0 * (float(np.float64(msv.sequence_transitions(Lc)[1])) -
                           float(np.float64(msv.sequence_transitions(40)[1])))
        # Z = Z_core move^2 (1 + r) with r the odds of the paths that emit a flank residue; their share f = r / (1 + r)
        # of Z is at most the summed special posteriors, and log(1 + r) <= r <= 2 f while f < 1/2
        flank1 = float((post[2] + post[3] + post[4]).sum())
        tol = 2.0 * (flank0 + flank1) + 1e-9
        assert flank1 < 0.25 and abs(predicted) > 8.0 * tol and abs((s1 - s0) - predicted) <= tol, \
            (Lc, s1 - s0, predicted, flank0, flank1)
        rows = post[0].sum(axis=1) + post[1].sum(axis=1) + post[2] + post[3] + post[4]
        assert np.max(np.abs(rows - 1.0)) <= 1e-9


def test_item_bytes_and_chunks():
    L = _native.lib()
    for S in (2, 6, 12, 22, 38):
        W = (S + 7) // 8
        for Le in (0, 1, 2, 64, 129):
            want = 4 * ((Le + 1) * 6 + Le * 2 * S * 64 + Le * (W * 64 + 1))
            assert L.msv_aln_item_bytes(S, Le) == want
    # the plan-cell layout of the Viterbi trace is the fill's: eight 4-bit cells a word, [row][word][lane]
    sizes = np.array([L.msv_aln_item_bytes(6, x) for x in (10, 20, 30, 5)], np.uint64)
    cuts, n = np.zeros(5, np.uint64), C.c_uint64()
    assert L.msv_vit_trace_chunk_cuts(sizes.ctypes.data, 4, int(sizes[1] + sizes[0]), cuts.ctypes.data, C.byref(n)) == 0
    assert n.value == 3 and cuts[:4].tolist() == [0, 2, 3, 4]
    assert L.msv_vit_trace_chunk_cuts(sizes.ctypes.data, 4, int(sizes.max()) - 1, cuts.ctypes.data, C.byref(n)) == 9


def test_argument_errors():
    model = base_model(5, 3, False)
    codes = np.array([1, 2, 3], np.uint8)
    assert align_lib.cpu_decode(model, codes, Lc=2)[0] == 1  # Lc < Le
    assert align_lib.cpu_decode(model, np.array([1, 20], np.uint8))[0] == 4
    assert align_lib.cpu_align(model, np.array([1, 20], np.uint8))[0] == 4
    assert align_lib.cpu_align(model, codes, Lc=1)[0] == 1
    st, score, *post = align_lib.cpu_decode(model, codes)
    post32 = [np.asarray(x, np.float32) for x in post]
    L = _native.lib()
    sc, nd, no = C.c_float(), C.c_uint32(), C.c_uint64()
    args = (*[x.ctypes.data for x in post32], model[2].ctypes.data, 6, *[float(x) for x in model[3]], 3, 3)
    assert L.msv_aln_oa(*args, C.byref(sc), C.byref(nd), C.byref(no), None, None, None) == 0
    doms = np.zeros(nd.value, _native.DOMAIN_DTYPE)
    ops = np.zeros(no.value, np.uint8)
    assert L.msv_aln_oa(*args, C.byref(sc), C.byref(nd), C.byref(no), doms.ctypes.data, ops.ctypes.data, None) == 1
    assert L.msv_aln_oa(*args, C.byref(sc), None, C.byref(no), None, None, None) == 1
    small = C.c_uint32(0)  # the second call with counts that are too small
    pp = np.zeros(no.value, np.float32)
    assert nd.value >= 1
    assert L.msv_aln_oa(*args, C.byref(sc), C.byref(small), C.byref(no), doms.ctypes.data, ops.ctypes.data,
                        pp.ctypes.data) == 1
    assert L.msv_aln_oa(None, *args[1:], C.byref(sc), C.byref(nd), C.byref(no), None, None, None) == 1
    with pytest.raises(ValueError):
        msv.aln_oa(post32[0][:, :3], *post32[1:], model[2], model[3])
