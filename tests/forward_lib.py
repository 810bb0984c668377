"""Shared by the Forward stage's tests: the score tables of a profile without a device, the library's
float64 CPU Forward through the C-ABI, an INDEPENDENT numpy float64 recurrence in log space (np.logaddexp, with
switches that remove one term of the model), the tolerance of msv.h, and raw device profiles over custom tables."""
import ctypes as C

import numpy as np

import hmm_fasta_viterbi_amd as msv
from hmm_fasta_viterbi_amd import _native

MM, MI, MD, IM, II, DM, DD = range(7)
U = 2.0 ** -24


def tolerance(L, leng, ref):
    """msv.h: |gpu - cpu64| <= 16 (L + LENG) 2^-24 + 4 2^-24 |cpu64| nats, per sequence."""
    return 16.0 * (np.asarray(L, np.float64) + leng) * U + 4.0 * U * np.abs(ref)


def tables(hmm, insert_mode=0):
    """(msc [20][M], isc [20][M] or None, tsc [M][7], (tr_B_Mk, tr_E_C, tr_E_J)) of a parsed profile."""
    M = hmm.model_length
    msc, isc, tsc = np.zeros((20, M), np.float32), np.zeros((20, M), np.float32), np.zeros((M, 7), np.float32)
    b, c, j = C.c_float(), C.c_float(), C.c_float()
    assert _native.lib().msv_hmm_viterbi_scores(hmm._h, insert_mode, msc.ctypes.data, isc.ctypes.data, tsc.ctypes.data,
                                                C.byref(b), C.byref(c), C.byref(j)) == 0
    return msc, (isc if insert_mode else None), tsc, (b.value, c.value, j.value)


def stress_transitions(tsc):
    """test_gpu_viterbi.py's stress transitions: d->d 0.995, m->d 0.9, d->m 0.3 -- D mass crosses many lanes."""
    t = tsc.copy()
    t[:, DD] = np.float32(np.log(np.float32(0.995)))
    t[:, MD] = np.float32(np.log(np.float32(0.9)))
    t[:, DM] = np.float32(np.log(np.float32(0.3)))
    return t


def distinct_exits(consts):
    return (consts[0], float(np.float32(consts[1]) - np.float32(0.75)), consts[2])


def _args(msc, isc, tsc, consts):
    return (msc.ctypes.data, None if isc is None else isc.ctypes.data, tsc.ctypes.data, msc.shape[1],
            *[float(x) for x in consts])


def cpu_score(msc, isc, tsc, consts, codes):
    """msv_fwd_cpu_score -> (status, float64 score)."""
    out = C.c_double()
    c = np.ascontiguousarray(codes, np.uint8)
    st = _native.lib().msv_fwd_cpu_score(*_args(msc, isc, tsc, consts), c.ctypes.data if c.size else None, len(c),
                                         C.byref(out))
    return st, out.value


def cpu_scores(msc, isc, tsc, consts, codes, offsets):
    """msv_fwd_cpu_score_batch -> float64 [n]."""
    codes = np.ascontiguousarray(codes, np.uint8)
    offsets = np.ascontiguousarray(offsets, np.uint64)
    out = np.zeros(len(offsets) - 1, np.float64)
    st = _native.lib().msv_fwd_cpu_score_batch(*_args(msc, isc, tsc, consts), codes.ctypes.data if codes.size else None,
                                               offsets.ctypes.data, len(out), out.ctypes.data)
    assert st == 0, st
    return out


def _window_logsumexp(x, w):
    """out[k] = log sum exp x[max(0, k-w+1) .. k], exactly (no difference of running sums, which would cancel
    where the window has lost the row's dominant term): blocks of w, a prefix and a suffix scan in each, and a
    window is the suffix of its first block joined to the prefix of its second."""
    n = len(x)
    nb = -(-n // w)
    blocks = np.full(nb * w, -np.inf)
    blocks[:n] = x
    blocks = blocks.reshape(nb, w)
    pre = np.logaddexp.accumulate(blocks, axis=1).ravel()
    suf = np.logaddexp.accumulate(blocks[:, ::-1], axis=1)[:, ::-1].ravel()
    k = np.arange(n)
    lo = np.maximum(k - w + 1, 0)
    whole = (lo % w == 0) & (k - lo == w - 1)  # the window is one block: its suffix alone
    return np.where(whole | (k < w), pre[k], np.logaddexp(suf[lo], pre[k]))


def np_forward(msc, isc, tsc, consts, codes, *, d_exits=True, inserts=True, j_loop=True, dm=True, d_reach=None,
               d_scan=False):
    """The model of msv.h in LOG space, float64, vectorised over k with np.logaddexp; the in-row D chain is a
    plain loop over the states (over the steps for a cut), or with d_scan one accumulate.  Switches remove one
    term each: the D -> E exits, the I states, the J loop, the d->m transitions;
    d_reach = r cuts every D chain after r d->d steps (D mass from more than r states upstream is dropped).
    d_scan = True restates the D chain for long models whose d->d are all finite: with P[j] the sum of d->d over
    nodes 1 .. j, D(k) = P[k-1] + log sum over sources s of exp(M(s) + m->d(s) - P[s]), s = k-1-r .. k-1 -- one
    np.logaddexp.accumulate (a windowed one for the cut) instead of a loop over states or over steps."""
    tBM, tEC, tEJ = (float(x) for x in consts)
    M = msc.shape[1]
    K = M - 1
    L = len(codes)
    if L == 0:
        return -np.inf
    loop, move = (float(x) for x in msv.sequence_transitions(L))
    la = np.logaddexp
    NI = -np.inf
    m = msc.astype(np.float64)
    ins = np.zeros((20, M)) if isc is None else isc.astype(np.float64)
    t = np.full((M, 7), NI)
    t[1:K] = tsc[1:K].astype(np.float64)  # nodes 1 .. LENG-1
    if not dm:
        t[:, DM] = NI
    Mp, Ip, Dp = (np.full(M, NI) for _ in range(3))
    N, J, Cc = 0.0, NI, NI
    B = move
    for i in range(L):
        r = codes[i]
        Mc, Ic, Dc = (np.full(M, NI) for _ in range(3))
        with np.errstate(invalid="ignore"):
            prev = la(la(Mp[:-1] + t[:-1, MM], Ip[:-1] + t[:-1, IM]), Dp[:-1] + t[:-1, DM])
            Mc[1:] = m[r, 1:] + la(prev, B + tBM)
            if inserts:
                Ic[1:K] = ins[r, 1:K] + la(Mp[1:K] + t[1:K, MI], Ip[1:K] + t[1:K, II])
        if d_scan:
            P = np.zeros(M)
            P[1:K] = np.cumsum(t[1:K, DD])
            P[K:] = P[K - 1] if K > 1 else 0.0
            x = Mc + t[:, MD] - P  # (node 0 and node LENG have no m->d: -inf)
            acc = np.logaddexp.accumulate(x) if d_reach is None else _window_logsumexp(x, d_reach + 1)
            Dc[2:] = acc[1:-1] + P[1:-1]
        elif d_reach is None:
            for k in range(2, M):
                Dc[k] = la(Mc[k - 1] + t[k - 1, MD], Dc[k - 1] + t[k - 1, DD])
        else:  # D(k) = sum over sources s = k-1, k-2, .. k-1-d_reach of M(s) tMD(s) prod tDD
            # source s = k-1-step enters D(s+1) by m->d of node s, then takes the d->d of nodes s+1 .. k-1:
            # P[j] = sum of d->d over nodes 1 .. j (finite in the models this is used on)
            src = Mc + t[:, MD]
            P = np.zeros(M)
            P[1:K] = np.cumsum(t[1:K, DD])
            for step in range(d_reach + 1):
                ks = np.arange(2 + step, M)
                if len(ks) == 0:
                    break
                Dc[ks] = la(Dc[ks], src[ks - 1 - step] + P[ks - 1] - P[ks - 1 - step])
        E = np.logaddexp.reduce(Mc[1:])
        if d_exits and M > 2:
            E = la(E, np.logaddexp.reduce(Dc[2:]))
        N = N + loop
        J = la(J + loop, E + tEJ) if j_loop else NI
        Cc = la(Cc + loop, E + tEC)
        B = la(N, J) + move
        Mp, Ip, Dp = Mc, Ic, Dc
    return Cc + move


def create_profile(msc, isc, tsc, consts, variant=None):
    """A raw msv_fwd_profile over custom tables (destroy with destroy_profile)."""
    p = C.c_void_p()
    st = _native.lib().msv_fwd_profile_create(0, *_args(msc, isc, tsc, consts), C.byref(p))
    assert st == 0, _native.STATUS.get(st, st)
    if variant is not None:
        st = _native.lib().msv_fwd_profile_set_variant(p, variant.encode())
        assert st == 0, (variant, _native.STATUS.get(st, st))
    return p


def destroy_profile(p):
    _native.lib().msv_fwd_profile_destroy(p)


def gpu_scores(p, codes, offsets):
    """msv_fwd_score_batch -> (status, float32 [n])."""
    codes = np.ascontiguousarray(codes, np.uint8)
    offsets = np.ascontiguousarray(offsets, np.uint64)
    out = np.zeros(len(offsets) - 1, np.float32)
    st = _native.lib().msv_fwd_score_batch(p, codes.ctypes.data if codes.size else None, offsets.ctypes.data,
                                           len(out), out.ctypes.data, None)
    return st, out


def assert_close(got, ref, offsets, leng, what=""):
    """Every finite score within msv.h's tolerance of the float64 reference; -inf, +inf and NaN classes equal.
    Prints the worst error against its bound before asserting."""
    got = np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    L = np.diff(np.asarray(offsets, np.uint64).astype(np.int64))
    fin = np.isfinite(ref)
    assert np.array_equal(np.isfinite(got), fin), (what, got[np.isfinite(got) != fin], ref[np.isfinite(got) != fin])
    assert np.array_equal(got[~fin], ref[~fin], equal_nan=True), (what, got[~fin], ref[~fin])
    err = np.abs(got[fin] - ref[fin])
    tol = tolerance(L[fin], leng, ref[fin])
    if err.size:
        w = int(np.argmax(err / tol))
        print(f"{what}: worst |gpu - cpu64| = {err[w]:.3e} nats (bound {tol[w]:.3e}, score {ref[fin][w]:.3f}), "
              f"max abs {err.max():.3e} over {err.size} sequences")
    bad = np.flatnonzero(err > tol)
    assert bad.size == 0, (what, err[bad][:5], tol[bad][:5], ref[fin][bad][:5])
