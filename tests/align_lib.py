"""Shared by the alignment stage's tests (test helper, not a conftest): the library's CPU functions
through the C-ABI over raw tables, the tolerances of msv.h, an explicit enumerator of every state path of a tiny
model that records each residue's label, and the device call on a raw profile."""
import ctypes as C

import numpy as np

import hmm_fasta_viterbi_amd as msv
from hmm_fasta_viterbi_amd import _native
from forward_lib import MM, MI, MD, IM, II, DM, DD, U, _args


def post_bound(Le, leng):
    """msv.h: |gpu - cpu64| <= 48 (Le + LENG) 2^-24 + 2 2^-24, absolute, for every posterior."""
    return 48.0 * (np.asarray(Le, np.float64) + leng) * U + 2.0 * U


def oa_bound(Le, leng):
    """msv.h: |gpu - cpu| <= Le (posterior bound) + Le^2 2^-24."""
    Le = np.asarray(Le, np.float64)
    return Le * post_bound(Le, leng) + Le * Le * U


def _ptr(a):
    return a.ctypes.data if a.size else None


def cpu_decode(model, codes, Lc=None):
    """msv_aln_cpu_decode -> (status, score, ppM, ppI, ppN, ppJ, ppC); ppM, ppI float64 [Le, LENG + 1]."""
    msc, isc, tsc, consts = model
    c = np.ascontiguousarray(codes, np.uint8)
    Le, M = len(c), msc.shape[1]
    sc = C.c_double()
    pm, pi = np.zeros((Le, M)), np.zeros((Le, M))
    pn, pj, pc = (np.zeros(Le) for _ in range(3))
    st = _native.lib().msv_aln_cpu_decode(*_args(msc, isc, tsc, consts), _ptr(c), Le, Le if Lc is None else Lc,
                                          C.byref(sc), _ptr(pm), _ptr(pi), _ptr(pn), _ptr(pj), _ptr(pc))
    return st, sc.value, pm, pi, pn, pj, pc


def cpu_align(model, codes, Lc=None):
    """msv_aln_cpu_align by its two calls -> (status, score, oa, domains, ops, op_pp)."""
    msc, isc, tsc, consts = model
    c = np.ascontiguousarray(codes, np.uint8)
    L = _native.lib()
    sc, oa, nd, no = C.c_double(), C.c_float(), C.c_uint32(), C.c_uint64()
    args = (*_args(msc, isc, tsc, consts), _ptr(c), len(c), len(c) if Lc is None else Lc)
    st = L.msv_aln_cpu_align(*args, C.byref(sc), C.byref(oa), C.byref(nd), C.byref(no), None, None, None)
    doms = np.zeros(nd.value if st == 0 else 0, _native.DOMAIN_DTYPE)
    ops = np.zeros(no.value if st == 0 else 0, np.uint8)
    pp = np.zeros(len(ops), np.float32)
    if st == 0 and nd.value:
        st = L.msv_aln_cpu_align(*args, C.byref(sc), C.byref(oa), C.byref(nd), C.byref(no), doms.ctypes.data,
                                 ops.ctypes.data, pp.ctypes.data)
    return st, sc.value, np.float32(oa.value), doms, ops, pp


def oa(model, post, Lc=None):
    """msv.aln_oa on (ppM, ppI, ppN, ppJ, ppC) of any float type, rounded to float32 once."""
    return msv.aln_oa(*[np.asarray(x, np.float32) for x in post], model[2], model[3], Lc)


def path_key(doms, ops):
    """A path as a tuple of domains, each a tuple of (state, k, i) with i relative to the arrays' own numbering."""
    out = []
    for d in doms:
        i, k = int(d["i_from"]) - 1, int(d["k_from"]) - 1
        dom = []
        for op in ops[int(d["ops_begin"]):int(d["ops_begin"]) + int(d["ops_len"])].tobytes():
            if op == 77:
                i, k = i + 1, k + 1
            elif op == 73:
                i += 1
            else:
                k += 1
            dom.append((chr(op), k, i))
        out.append(tuple(dom))
    return tuple(out)


def labels_of(key, Le):
    """Per residue 1 .. Le the label of the path `key`: ('M', k), ('I', k), 'N', 'J' or 'C'."""
    lab = [None] * (Le + 1)
    for dom in key:
        for st, k, i in dom:
            if st != "D":
                lab[i] = (st, k)
    firsts = [dom[0][2] for dom in key]
    lasts = [max(i for _, _, i in dom) for dom in key]
    for i in range(1, Le + 1):
        if lab[i] is None:
            lab[i] = "N" if not key or i < firsts[0] else "C" if i > lasts[-1] else "J"
    return lab[1:]


def enumerate_paths(model, codes, Lc=None):
    """Every state path of msv.h's Forward model over `codes` with odds > 0, explicitly: {path key: odds}, float64.
    Tiny models only."""
    msc, isc, tsc, consts = model
    K = msc.shape[1] - 1
    L = len(codes)
    loop, move = (float(np.exp(np.float64(x))) for x in msv.sequence_transitions(L if Lc is None else Lc))
    tBM, tEC, tEJ = (float(np.exp(np.float64(x))) for x in consts)
    with np.errstate(under="ignore"):
        em = np.exp(msc.astype(np.float64))
        ei = np.ones_like(em) if isc is None else np.exp(isc.astype(np.float64))
        t = np.zeros((K + 1, 7))
        t[1:K] = np.exp(tsc[1:K].astype(np.float64))
    paths = {}

    def emit_m(k, i):
        return em[codes[i], k]

    def core(st, k, i, w, dom, done):
        """In core state (st, k) having consumed i residues, odds w so far."""
        if w == 0.0:
            return
        if st == "M" or (st == "D" and k >= 2):
            special("E", i, w, done + (tuple(dom),))
        if k < K:
            if st in "MD" and i < L:
                core("M", k + 1, i + 1, w * t[k, MM if st == "M" else DM] * emit_m(k + 1, i), dom + [("M", k + 1, i + 1)],
                     done)
            if st in "MD":
                core("D", k + 1, i, w * t[k, MD if st == "M" else DD], dom + [("D", k + 1, i)], done)
            if st == "M" and i < L:
                core("I", k, i + 1, w * t[k, MI] * ei[codes[i], k], dom + [("I", k, i + 1)], done)
            if st == "I":
                if i < L:
                    core("M", k + 1, i + 1, w * t[k, IM] * emit_m(k + 1, i), dom + [("M", k + 1, i + 1)], done)
                    core("I", k, i + 1, w * t[k, II] * ei[codes[i], k], dom + [("I", k, i + 1)], done)

    def special(st, i, w, done):
        if w == 0.0:
            return
        if st == "E":
            special("C", i, w * tEC, done)
            special("J", i, w * tEJ, done)
        elif st == "C":
            if i == L:
                paths[done] = paths.get(done, 0.0) + w * move
            else:
                special("C", i + 1, w * loop, done)
        else:  # N or J: loop, or move to B and enter any node
            if i < L:
                special(st, i + 1, w * loop, done)
                for k in range(1, K + 1):
                    core("M", k, i + 1, w * move * tBM * emit_m(k, i), [("M", k, i + 1)], done)

    special("N", 0, 1.0, ())
    return paths


def enumerated_posteriors(paths, Le, M):
    """(Z, ppM, ppI, ppN, ppJ, ppC) summed over the enumerated paths."""
    Z = sum(paths.values())
    pm, pi = np.zeros((Le, M)), np.zeros((Le, M))
    pn, pj, pc = (np.zeros(Le) for _ in range(3))
    for key, w in paths.items():
        for i, lab in enumerate(labels_of(key, Le)):
            if lab == "N":
                pn[i] += w
            elif lab == "J":
                pj[i] += w
            elif lab == "C":
                pc[i] += w
            elif lab[0] == "M":
                pm[i, lab[1]] += w
            else:
                pi[i, lab[1]] += w
    return Z, pm / Z, pi / Z, pn / Z, pj / Z, pc / Z


def path_accuracy(key, post):
    """The summed posteriors of the labels of path `key` (float64)."""
    pm, pi, pn, pj, pc = post
    total = 0.0
    for i, lab in enumerate(labels_of(key, len(pn))):
        total += {"N": pn, "J": pj, "C": pc}[lab][i] if isinstance(lab, str) else (pm if lab[0] == "M" else pi)[i, lab[1]]
    return total


# ---- the device, on a raw msv_dom_profile (decode_lib.create_profile) ---------------------------------------------

def gpu_align(p, M, codes, offsets, items, workspace_bytes=0, keep=True):
    """msv_aln_align_batch on a raw profile -> (status, dict or None): env, oa, dom_off, domains, ops, op_pp, stats and,
    with keep, post[q] = (ppM, ppI, ppN, ppJ, ppC)."""
    codes = np.ascontiguousarray(codes, np.uint8)
    offsets = np.ascontiguousarray(offsets, np.uint64)
    it = np.zeros(len(items), _native.ITEM_DTYPE)
    for q, (s, a, b) in enumerate(items):
        it[q] = (s, a, b)
    L = _native.lib()
    r = C.c_void_p()
    st = L.msv_aln_align_batch(p, _ptr(codes), offsets.ctypes.data, len(offsets) - 1, _ptr(it), len(it),
                               workspace_bytes, 1 if keep else 0, C.byref(r))
    if not r.value:
        return st, None
    try:
        m = L.msv_aln_result_count(r)
        out = {"env": np.zeros(m, np.float32), "oa": np.zeros(m, np.float32), "dom_off": np.zeros(m + 1, np.uint64),
               "domains": np.zeros(L.msv_aln_result_domains(r), _native.DOMAIN_DTYPE),
               "ops": np.zeros(L.msv_aln_result_ops(r), np.uint8)}
        out["op_pp"] = np.zeros(len(out["ops"]), np.float32)
        assert L.msv_aln_result_copy(r, out["env"].ctypes.data, out["oa"].ctypes.data, out["dom_off"].ctypes.data,
                                     _ptr(out["domains"]), _ptr(out["ops"]), _ptr(out["op_pp"])) == 0
        stats = _native.AlnStats()
        assert L.msv_aln_result_stats(r, C.byref(stats)) == 0
        out["stats"] = {f: getattr(stats, f) for f, _ in stats._fields_}
        if keep and st in (0, 4):
            out["post"] = []
            for q in range(m):
                Le = int(it["i_to"][q]) - int(it["i_from"][q]) + 1
                pm, pi = np.zeros((Le, M), np.float32), np.zeros((Le, M), np.float32)
                pn, pj, pc = (np.zeros(Le, np.float32) for _ in range(3))
                assert L.msv_aln_result_posteriors(r, q, _ptr(pm), _ptr(pi), _ptr(pn), _ptr(pj), _ptr(pc)) == 0
                out["post"].append((pm, pi, pn, pj, pc))
    finally:
        L.msv_aln_result_free(r)
    return st, out


def item_domains(out, q):
    """(domains, ops, op_pp) of item q with ops_begin rebased to 0."""
    lo, hi = int(out["dom_off"][q]), int(out["dom_off"][q + 1])
    doms = out["domains"][lo:hi].copy()
    if len(doms) == 0:
        return doms, np.zeros(0, np.uint8), np.zeros(0, np.float32)
    o0 = int(doms["ops_begin"][0])
    o1 = int(doms["ops_begin"][-1]) + int(doms["ops_len"][-1])
    doms["ops_begin"] -= np.uint64(o0)
    return doms, out["ops"][o0:o1], out["op_pp"][o0:o1]
