"""Shared by the domain stage's tests (test helper, not a conftest): the library's float64 CPU decode
through the C-ABI over raw tables, an INDEPENDENT numpy float64 restatement in log space with full matrices (so that
occ can be checked against sum_k fM bM + fI bI, and one term of the model can be removed), the tolerances of msv.h, and
raw device profiles over custom tables."""
import ctypes as C

import numpy as np

import hmm_fasta_viterbi_amd as msv
from hmm_fasta_viterbi_amd import _native
from forward_lib import MM, MI, MD, IM, II, DM, DD, U, _args

RT1, RT2 = 0.25, 0.10


def post_tolerance(L, leng):
    """msv.h: |gpu - cpu64| <= 48 (L + LENG) 2^-24 + 8 2^-24, absolute, for begin, end and occ."""
    return 48.0 * (np.asarray(L, np.float64) + leng) * U + 8.0 * U


def cpu_decode(msc, isc, tsc, consts, codes):
    """msv_dom_cpu_decode -> (status, forward score, backward score, begin, end, occ), the arrays float64 [L]."""
    c = np.ascontiguousarray(codes, np.uint8)
    f, b = C.c_double(), C.c_double()
    begin, end, occ = (np.zeros(len(c), np.float64) for _ in range(3))
    ptr = lambda a: a.ctypes.data if a.size else None
    st = _native.lib().msv_dom_cpu_decode(*_args(msc, isc, tsc, consts), ptr(c), len(c), C.byref(f), C.byref(b),
                                          ptr(begin), ptr(end), ptr(occ))
    return st, f.value, b.value, begin, end, occ


def cpu_decode_batch(msc, isc, tsc, consts, codes, offsets):
    """msv_dom_cpu_decode_batch -> (forward scores, backward scores, begin, end, occ), per-residue arrays indexed
    from the batch's first residue."""
    codes = np.ascontiguousarray(codes, np.uint8)
    offsets = np.ascontiguousarray(offsets, np.uint64)
    n = len(offsets) - 1
    total = int(offsets[-1] - offsets[0])
    f, b = np.zeros(n, np.float64), np.zeros(n, np.float64)
    begin, end, occ = (np.zeros(total, np.float64) for _ in range(3))
    ptr = lambda a: a.ctypes.data if a.size else None
    st = _native.lib().msv_dom_cpu_decode_batch(*_args(msc, isc, tsc, consts), ptr(codes), offsets.ctypes.data, n,
                                                f.ctypes.data, b.ctypes.data, ptr(begin), ptr(end), ptr(occ))
    assert st == 0, st
    return f, b, begin, end, occ


def np_decode(msc, isc, tsc, consts, codes, row_L_chain=True):
    """The model of msv.h in LOG space, float64, with the full Forward and Backward matrices.  Returns a dict:
    fwd, bck (nats), begin, end, occ [L] as msv.h defines them on the specials, and occ_core = sum_k (fM bM + fI bI)
    / Z, the same probability counted on the core states.  row_L_chain=False leaves the silent D chain out of row L
    (bD(L,k) = [k>=2] bE, bM(L,k) = bE): the mistake the tests must be able to see."""
    tBM, tEC, tEJ = (float(x) for x in consts)
    M = msc.shape[1]
    K = M - 1
    L = len(codes)
    loop, move = (float(x) for x in msv.sequence_transitions(L))
    la = np.logaddexp
    NI = -np.inf
    m = msc.astype(np.float64)
    ins = np.zeros((20, M)) if isc is None else isc.astype(np.float64)
    t = np.full((M + 1, 7), NI)
    t[1:K] = tsc[1:K].astype(np.float64)  # nodes 1 .. LENG-1
    with np.errstate(invalid="ignore"):
        fM, fI, fD = (np.full((L + 1, M + 2), NI) for _ in range(3))
        fN, fJ, fC, fB, fE = (np.full(L + 1, NI) for _ in range(5))
        fN[0], fB[0] = 0.0, move
        for i in range(1, L + 1):
            r = codes[i - 1]
            for k in range(1, K + 1):
                fM[i, k] = m[r, k] + la(la(la(fM[i - 1, k - 1] + t[k - 1, MM], fI[i - 1, k - 1] + t[k - 1, IM]),
                                           fD[i - 1, k - 1] + t[k - 1, DM]), fB[i - 1] + tBM)
                if k < K:
                    fI[i, k] = ins[r, k] + la(fM[i - 1, k] + t[k, MI], fI[i - 1, k] + t[k, II])
                if k >= 2:
                    fD[i, k] = la(fM[i, k - 1] + t[k - 1, MD], fD[i, k - 1] + t[k - 1, DD])
            fE[i] = la(np.logaddexp.reduce(fM[i, 1:K + 1]), np.logaddexp.reduce(fD[i, 2:K + 1]) if K >= 2 else NI)
            fN[i] = fN[i - 1] + loop
            fJ[i] = la(fJ[i - 1] + loop, fE[i] + tEJ)
            fC[i] = la(fC[i - 1] + loop, fE[i] + tEC)
            fB[i] = la(fN[i], fJ[i]) + move
        Z = fC[L] + move
        bM, bI, bD = (np.full((L + 2, M + 2), NI) for _ in range(3))
        bN, bJ, bC, bB, bE = (np.full(L + 2, NI) for _ in range(5))
        bC[L] = move
        bE[L] = tEC + bC[L]
        for k in range(K, 0, -1):
            if row_L_chain:
                bD[L, k] = la(bE[L] if k >= 2 else NI, t[k, DD] + bD[L, k + 1])
                bM[L, k] = la(bE[L], t[k, MD] + bD[L, k + 1])
            else:
                bD[L, k] = bE[L] if k >= 2 else NI
                bM[L, k] = bE[L]
        for i in range(L - 1, -1, -1):
            r = codes[i]
            bB[i] = tBM + np.logaddexp.reduce(m[r, 1:K + 1] + bM[i + 1, 1:K + 1])
            bJ[i] = la(loop + bJ[i + 1], move + bB[i])
            bC[i] = loop + bC[i + 1]
            bN[i] = la(loop + bN[i + 1], move + bB[i])
            bE[i] = la(tEJ + bJ[i], tEC + bC[i])
            if i == 0:
                break
            for k in range(K, 0, -1):
                g = m[r, k + 1] + bM[i + 1, k + 1] if k < K else NI
                h = ins[r, k] + bI[i + 1, k] if k < K else NI
                bD[i, k] = la(la(bE[i] if k >= 2 else NI, t[k, DM] + g), t[k, DD] + bD[i, k + 1])
                bM[i, k] = la(la(la(bE[i], t[k, MM] + g), t[k, MI] + h), t[k, MD] + bD[i, k + 1])
                bI[i, k] = la(t[k, IM] + g, t[k, II] + h)
        idx = np.arange(1, L + 1)
        begin = np.exp(fB[idx - 1] + bB[idx - 1] - Z)
        end = np.exp(fE[idx] + bE[idx] - Z)
        occ = 1.0 - np.exp(loop + la(la(fN[idx - 1] + bN[idx], fJ[idx - 1] + bJ[idx]), fC[idx - 1] + bC[idx]) - Z)
        core = np.logaddexp.reduce(np.logaddexp(fM[1:L + 1, 1:K + 1] + bM[1:L + 1, 1:K + 1],
                                                fI[1:L + 1, 1:K + 1] + bI[1:L + 1, 1:K + 1]), axis=1)
        occ_core = np.exp(core - Z)
    return {"fwd": Z, "bck": bN[0], "begin": begin, "end": end, "occ": occ, "occ_core": occ_core}


def np_regions(begin, end, occ, rt1=RT1, rt2=RT2):
    """The envelope rule of msv.h restated in Python on arrays of any float type -> [(i_from, i_to)]."""
    out, start, trig = [], 0, False
    for j in range(1, len(occ) + 1):
        if not trig:
            if occ[j - 1] - begin[j - 1] < rt2:
                start = j
            elif start == 0:
                start = j
            if occ[j - 1] >= rt1:
                trig = True
        elif occ[j - 1] - end[j - 1] < rt2:
            out.append((start, j))
            start, trig = 0, False
    return out


def rule_margin(begin, end, occ, rt1=RT1, rt2=RT2):
    """The smallest distance of any comparison the rule makes on these (float64) arrays from its threshold: the
    comparisons made depend on the state, so the rule is walked."""
    worst, start, trig = np.inf, 0, False
    for j in range(1, len(occ) + 1):
        o = occ[j - 1]
        if not trig:
            worst = min(worst, abs(o - begin[j - 1] - rt2), abs(o - rt1))
            if o - begin[j - 1] < rt2:
                start = j
            elif start == 0:
                start = j
            if o >= rt1:
                trig = True
        else:
            worst = min(worst, abs(o - end[j - 1] - rt2))
            if o - end[j - 1] < rt2:
                start, trig = 0, False
    return worst


# ---- raw device profiles ---------------------------------------------------------------------------------------

def create_profile(msc, isc, tsc, consts, variant=None):
    """A raw msv_dom_profile over custom tables (destroy with destroy_profile)."""
    p = C.c_void_p()
    st = _native.lib().msv_dom_profile_create(0, *_args(msc, isc, tsc, consts), C.byref(p))
    assert st == 0, _native.STATUS.get(st, st)
    if variant is not None:
        st = _native.lib().msv_dom_profile_set_variant(p, variant.encode())
        assert st == 0, (variant, _native.STATUS.get(st, st))
    return p


def destroy_profile(p):
    _native.lib().msv_dom_profile_destroy(p)


def describe(p):
    info = _native.DomInfo()
    assert _native.lib().msv_dom_profile_describe(p, C.byref(info)) == 0
    return info.as_dict()


def gpu_scores(p, codes, offsets):
    """msv_dom_score_batch -> (status, float32 [n]): the recording kernel's Forward score."""
    codes = np.ascontiguousarray(codes, np.uint8)
    offsets = np.ascontiguousarray(offsets, np.uint64)
    out = np.zeros(len(offsets) - 1, np.float32)
    st = _native.lib().msv_dom_score_batch(p, codes.ctypes.data if codes.size else None, offsets.ctypes.data,
                                           len(out), out.ctypes.data, None)
    return st, out


def gpu_decode(p, codes, offsets, select=None, rt1=RT1, rt2=RT2, workspace_bytes=0):
    """msv_dom_decode_batch on a raw profile -> (status, msv.Envelopes or None)."""
    codes = np.ascontiguousarray(codes, np.uint8)
    offsets = np.ascontiguousarray(offsets, np.uint64)
    n = len(offsets) - 1
    sel = None if select is None else np.ascontiguousarray(select, np.uint32)
    sel_buf = sel if sel is None or sel.size else np.zeros(1, np.uint32)
    L = _native.lib()
    r = C.c_void_p()
    st = L.msv_dom_decode_batch(p, codes.ctypes.data if codes.size else None, offsets.ctypes.data, n,
                                None if sel is None else sel_buf.ctypes.data, 0 if sel is None else sel.size,
                                rt1, rt2, workspace_bytes, C.byref(r))
    if not r.value:
        return st, None
    try:
        m = L.msv_dom_result_count(r)
        fwd, bck = np.zeros(m, np.float32), np.zeros(m, np.float32)
        res_off, reg_off = np.zeros(m + 1, np.uint64), np.zeros(m + 1, np.uint64)
        begin, end, occ = (np.zeros(L.msv_dom_result_residues(r), np.float32) for _ in range(3))
        regions = np.zeros(L.msv_dom_result_regions(r), _native.REGION_DTYPE)
        ptr = lambda a: a.ctypes.data if a.size else None
        assert L.msv_dom_result_copy(r, fwd.ctypes.data, bck.ctypes.data, res_off.ctypes.data, ptr(begin), ptr(end),
                                     ptr(occ), reg_off.ctypes.data, ptr(regions)) == 0
        stats = _native.DomStats()
        assert L.msv_dom_result_stats(r, C.byref(stats)) == 0
    finally:
        L.msv_dom_result_free(r)
    return st, msv.Envelopes(np.arange(n, dtype=np.uint32) if sel is None else sel, fwd, bck, res_off, begin, end,
                             occ, reg_off, regions, status=_native.STATUS.get(st, str(st)),
                             stats={f: getattr(stats, f) for f, _ in stats._fields_ if f != "reserved"})


def assert_posteriors_close(env, ref, offsets, leng, what=""):
    """Every posterior of every entry of `env` (whole-batch decode, entry q = sequence q) within msv.h's tolerance of
    the float64 reference `ref` = cpu_decode_batch(...)'s (fwd, bck, begin, end, occ).  Prints the worst error
    against its bound before asserting; returns it."""
    off = np.asarray(offsets, np.uint64).astype(np.int64)
    off = off - off[0]
    L = np.diff(off)
    assert np.array_equal(env.residue_offsets.astype(np.int64), off)
    tol = np.repeat(post_tolerance(L, leng), L)
    worst, which = 0.0, ""
    for name, got, want in (("begin", env.begin, ref[2]), ("end", env.end, ref[3]), ("occ", env.occ, ref[4])):
        err = np.abs(got.astype(np.float64) - want)
        if err.size:
            w = int(np.argmax(err / tol))
            if err[w] / tol[w] >= worst:
                worst, which = err[w] / tol[w], f"{name} {err[w]:.3e} (bound {tol[w]:.3e})"
            bad = np.flatnonzero(~(err <= tol))
            assert bad.size == 0, (what, name, bad[:5], err[bad][:5], tol[bad][:5])
    print(f"{what}: worst posterior error {which}: {worst:.4f} of the bound, over {len(tol)} residues")
    return worst
