"""Shared by the bias stage's tests (test helper, not a conftest): the library's host functions through
the C-ABI over raw tables, the tolerances of msv.h's "Bias stage" block, null2 from an explicit enumeration of every
state path of a tiny model, the item lists the GPU tests run (built without a GPU, so that a CPU test can assert the
input condition of the domcorrection bound on every item of them), and the device call with options."""
import ctypes as C
import functools

import numpy as np

from hmm_fasta_viterbi_amd import _native
from hmm_fasta_viterbi_amd.synthetic import concat_batches, random_batch
from align_lib import enumerate_paths, labels_of
from forward_batches import aimed_batch, base_model, consensus
from forward_lib import U, _args
from state_batches import _csr

R = 16  # msv_aln_info.null2_row_block; test_gpu_null2 asserts the library reports this value
OMEGA = 1.0 / 256.0


def _ptr(a):
    return a.ctypes.data if a.size else None


# ---- the host functions -------------------------------------------------------------------------------------------

def cpu_null2(model, codes, Lc=None):
    """msv_aln_cpu_null2 -> (status, null2 float64 [20], domcorrection)."""
    msc, isc, tsc, consts = model
    c = np.ascontiguousarray(codes, np.uint8)
    n2, dc = np.zeros(20), C.c_double()
    st = _native.lib().msv_aln_cpu_null2(*_args(msc, isc, tsc, consts), _ptr(c), len(c), len(c) if Lc is None else Lc,
                                         n2.ctypes.data, C.byref(dc))
    return st, n2, dc.value


def correction(null2, codes):
    """msv_aln_null2_correction on a float32 vector -> (status, float32)."""
    v = np.ascontiguousarray(null2, np.float32)
    c = np.ascontiguousarray(codes, np.uint8)
    out = C.c_float()
    st = _native.lib().msv_aln_null2_correction(v.ctypes.data, _ptr(c), len(c), C.byref(out))
    return st, np.float32(out.value)


def bias_scores(env, Le, Lc, dc, tau, lam, parent=None, fwd=None, lengths=None):
    """msv_aln_bias_scores -> (status, dict)."""
    env, dc = np.ascontiguousarray(env, np.float32), np.ascontiguousarray(dc, np.float32)
    Le, Lc = np.ascontiguousarray(Le, np.uint64), np.ascontiguousarray(Lc, np.uint64)
    m = len(env)
    out = {"dombias": np.zeros(m, np.float32), "domain_bits": np.zeros(m, np.float32), "domain_pvalues": np.zeros(m)}
    n_seq = 0
    args = [None, None, None]
    tail = [None, None, None]
    if fwd is not None:
        fwd, lengths = np.ascontiguousarray(fwd, np.float32), np.ascontiguousarray(lengths, np.uint64)
        parent = np.ascontiguousarray(parent, np.uint32)
        n_seq = len(fwd)
        out.update(seq_bias=np.zeros(n_seq, np.float32), seq_bits=np.zeros(n_seq, np.float32),
                   seq_pvalues=np.zeros(n_seq))
        args = [_ptr(parent), _ptr(fwd), _ptr(lengths)]
        tail = [_ptr(out[k]) for k in ("seq_bias", "seq_bits", "seq_pvalues")]
    st = _native.lib().msv_aln_bias_scores(_ptr(env), _ptr(Le), _ptr(Lc), _ptr(dc), m, args[0], args[1], args[2],
                                           n_seq, tau, lam, _ptr(out["dombias"]), _ptr(out["domain_bits"]),
                                           _ptr(out["domain_pvalues"]), *tail)
    return st, out


# ---- the model's float32 odds and the tolerances of msv.h ----------------------------------------------------------

def odds32(model):
    """(m, ins) float64 [20, LENG + 1]: the float32 odds the device tables hold (column 0 zeros; ins 1 for
    k = 1 .. LENG-1 without insert scores, 0 at LENG: the model has no insert state there)."""
    msc, isc = model[0], model[1]
    M = msc.shape[1]
    with np.errstate(under="ignore"):
        m = np.exp(msc.astype(np.float64)).astype(np.float32).astype(np.float64)
        ins = np.ones((20, M)) if isc is None else np.exp(isc.astype(np.float64)).astype(np.float32).astype(np.float64)
    m[:, 0] = 0.0
    ins[:, 0] = 0.0
    ins[:, M - 1] = 0.0
    return m, ins


def weights(model):
    """W_x = sum_k m[x][k] + sum_k ins[x][k] + 3."""
    m, ins = odds32(model)
    return m.sum(axis=1) + ins.sum(axis=1) + 3.0


def null2_bound(model, Le, null2_cpu):
    """msv.h: delta_x = (48 (Le + LENG) + 2 (Le + 2 LENG + 8)) 2^-24 null2_cpu[x] + W_x 2^-60."""
    leng = model[0].shape[1] - 1
    return (48.0 * (Le + leng) + 2.0 * (Le + 2.0 * leng + 8.0)) * U * np.asarray(null2_cpu) + weights(model) * 2.0 ** -60


def condition_holds(codes, null2_cpu, delta):
    """The input condition of the domcorrection bound: delta_x <= null2_cpu[x] / 2 for every x that occurs."""
    occ = np.bincount(np.asarray(codes, np.int64), minlength=20)[:20] > 0
    return bool(np.all(delta[occ] <= null2_cpu[occ] / 2.0))


def domcorr_bound(codes, null2_cpu, delta, dc_cpu):
    """msv.h: sum_x n_x delta_x / (null2_cpu[x] - delta_x) + 2^-24 (|dc_cpu| + that sum) + 2^-149."""
    n = np.bincount(np.asarray(codes, np.int64), minlength=20)[:20].astype(np.float64)
    occ = n > 0
    assert condition_holds(codes, null2_cpu, delta)
    moved = float(np.sum(n[occ] * delta[occ] / (null2_cpu[occ] - delta[occ])))
    return moved + U * (abs(dc_cpu) + moved) + 2.0 ** -149


def enumerated_null2(model, codes, Lc=None):
    """null2 float64 [20] from the enumeration of every state path: the expected emission count of each state,
    weighted by path odds -- independent of Forward / Backward."""
    M = model[0].shape[1]
    Le = len(codes)
    paths = enumerate_paths(model, codes, Lc)
    Z = sum(paths.values())
    eM, eI, eX = np.zeros(M), np.zeros(M), 0.0
    for key, w in paths.items():
        for lab in labels_of(key, Le):
            if isinstance(lab, str):
                eX += w
            elif lab[0] == "M":
                eM[lab[1]] += w
            else:
                eI[lab[1]] += w
    m, ins = odds32(model)
    return (m @ (eM / Z) + ins @ (eI / Z) + eX / Z) / Le


# ---- the GPU tests' item lists (built on the host) ----------------------------------------------------------------

def stretch(model, L, seed):
    """A sequence of exactly L residues made of consensus runs (every row carries mass)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    leng = model[0].shape[1] - 1
    parts, have = [], 0
    while have < L:
        core = min(20, leng, L - have)
        start = int(rng.integers(1, leng - core + 2))
        parts.append(consensus(model, start, start + core - 1))
        have += core
    return np.concatenate(parts)


def take(batch, idx):
    return _csr([batch[0][int(batch[1][i]):int(batch[1][i + 1])] for i in idx])


BLOCK_EDGES = (1, 2, R - 1, R, R + 1, 2 * R + 1)
LONGEST = 4 * R + 3


def model_lengths(S):
    return 64 * S, 64 * S - 1, 64 * (S - 2) + 1


def null2_items(model, S):
    """(codes, offsets, items, bad): homologs aimed at the lane edges (forward_batches.aimed_batch: tails, heads and
    windows at the capacity edge), envelopes of exactly 1, 2, R - 1, R, R + 1 and 2 R + 1 residues and one of 4 R + 3,
    every sequence whole; then one envelope cut from the middle of the longest (i_from > 1, Lc > Le), the first item
    again, and item `bad`, a whole sequence with one residue outside the 20."""
    leng = model[0].shape[1] - 1
    blocks = _csr([stretch(model, L, 900 + L) for L in BLOCK_EDGES + (LONGEST,)])
    if leng >= 24:
        aimed, where = aimed_batch(model, S, 32)
        pick = np.concatenate([where["tail"][::8], where["head"][::8],
                               where.get("window", np.zeros(0, np.int64))[::2]])
        batch = concat_batches(take(aimed, pick.astype(np.int64)), blocks)
    else:
        batch = concat_batches(random_batch(34, 4, 1, 40), blocks)
    spoiled = stretch(model, R + 5, 977).copy()
    spoiled[R + 1] = 21
    codes, offsets = concat_batches(batch, _csr([spoiled]))
    n = len(offsets) - 1
    L = np.diff(offsets.astype(np.int64))
    items = [(s, 1, int(L[s])) for s in range(n - 1) if L[s] > 0]
    items.append((n - 2, R - 3, 3 * R + 2))  # rows R-4 .. 3R+1 of the longest: no block of it starts where one did
    items.append(items[0])
    items.append((n - 1, 1, int(L[n - 1])))
    return codes, offsets, items, len(items) - 1


@functools.lru_cache(maxsize=None)
def case(S, isc, which):
    """(model, codes, offsets, items, bad, refs) of one of a variant shape's three models; refs[q] = (null2_cpu,
    domcorrection_cpu) of msv_aln_cpu_null2, None for the bad item.  Computed once and shared; do not modify."""
    leng = model_lengths(S)[which]
    model = base_model(leng, 51 + which, isc)
    codes, offsets, items, bad = null2_items(model, S)
    off = offsets.astype(np.int64)
    refs = []
    for q, (s, a, b) in enumerate(items):
        if q == bad:
            refs.append(None)
            continue
        st, n2, dc = cpu_null2(model, codes[off[s] + a - 1:off[s] + b], int(off[s + 1] - off[s]))
        assert st == 0
        refs.append((n2, dc))
    return model, codes, offsets, items, bad, refs


# ---- the device, on a raw msv_dom_profile (decode_lib.create_profile) ----------------------------------------------

def gpu_align_opts(p, M, codes, offsets, items, workspace_bytes=0, keep=False, null2=True, options=True):
    """msv_aln_align_batch_opts on a raw profile -> (status, dict or None): align_lib.gpu_align's dict plus, with
    null2, `null2` float32 [m, 20], `domcorr` float32 [m] and `null2_stats`; `null2_status` is what
    msv_aln_result_null2 answered.  options=False passes NULL options."""
    codes = np.ascontiguousarray(codes, np.uint8)
    offsets = np.ascontiguousarray(offsets, np.uint64)
    it = np.zeros(len(items), _native.ITEM_DTYPE)
    for q, (s, a, b) in enumerate(items):
        it[q] = (s, a, b)
    L = _native.lib()
    r = C.c_void_p()
    opts = _native.AlnOptions(workspace_bytes, 1 if keep else 0, 1 if null2 else 0)
    st = L.msv_aln_align_batch_opts(p, _ptr(codes), offsets.ctypes.data, len(offsets) - 1, _ptr(it), len(it),
                                    C.byref(opts) if options else None, C.byref(r))
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
        n2, dc = np.zeros((m, 20), np.float32), np.zeros(m, np.float32)
        out["null2_status"] = L.msv_aln_result_null2(r, _ptr(n2), _ptr(dc))
        if out["null2_status"] == 0:
            out["null2"], out["domcorr"] = n2, dc
            ns = _native.AlnNull2Stats()
            assert L.msv_aln_result_null2_stats(r, C.byref(ns)) == 0
            out["null2_stats"] = {f: getattr(ns, f) for f, _ in ns._fields_ if f != "struct_size"}
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
