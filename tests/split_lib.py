"""Shared by the split stage's tests (test helper, not a conftest): the library's CPU functions through
the C-ABI over raw tables, the float64 twin's matrix as the float32 arrays the definition takes, the batches whose
weight tests/test_split_batches.py shows on the CPU, and the device call on a raw profile."""
import ctypes as C

import numpy as np

import hmm_fasta_viterbi_amd as msv
from hmm_fasta_viterbi_amd import _native
from forward_batches import base_model, consensus
from forward_lib import U, _args
from state_batches import _csr

SEED = 42


def f_bound(Le, leng):
    """msv.h: every stored f within the relative 16 (Le + LENG) 2^-24 of the float64 twin."""
    return 16.0 * (Le + leng) * U


def _ptr(a):
    return a.ctypes.data if a.size else None


def cpu_forward(model, codes, Lc=None):
    """msv_spl_cpu_forward -> (status, score, fM, fI, fD float64 [Le, M], specials [Le + 1, 5], exponents [Le + 1])."""
    msc, isc, tsc, consts = model
    c = np.ascontiguousarray(codes, np.uint8)
    Le, M = len(c), msc.shape[1]
    sc = C.c_double()
    fm, fi, fd = (np.zeros((Le, M)) for _ in range(3))
    sp, ex = np.zeros((Le + 1, 5)), np.zeros(Le + 1, np.int32)
    st = _native.lib().msv_spl_cpu_forward(*_args(msc, isc, tsc, consts), _ptr(c), Le, Le if Lc is None else Lc,
                                           C.byref(sc), _ptr(fm), _ptr(fi), _ptr(fd), sp.ctypes.data, ex.ctypes.data)
    return st, sc.value, fm, fi, fd, sp, ex


def device_exponents(sp, ex):
    """The exponents the device would record for the twin's rows, by its rule (p7_forward_row.inc): a row whose E, in
    the scale so far, has passed 2^32 moves the scale up by floor(log2 E).  Also the least |log2 E - 32| over the
    rows: how far the nearest row is from falling on the other side of the rule under another rounding."""
    e = np.zeros(len(sp), np.int64)
    cur, margin = 0, np.inf
    for i in range(len(sp)):
        if sp[i, 4] > 0:
            lg = float(np.log2(sp[i, 4])) + int(ex[i]) - cur
            margin = min(margin, abs(lg - 32.0))
            if lg > 32.0:
                cur += int(np.floor(lg))
        e[i] = cur
    return e, margin


def as_float32(fm, fi, fd, sp, ex):
    """The twin's matrix rounded to float32 once, in the arrays msv_spl_sample takes.  The twin rescales at 2^256,
    beyond float32: every row is first moved, exactly, to the exponent the device's rule gives it
    (device_exponents).  On the tiny models of the path tests every exponent is 0 and nothing moves."""
    e, _ = device_exponents(sp, ex)
    shift = (ex.astype(np.int64) - e).astype(np.int32)
    with np.errstate(under="ignore"):
        sp32 = np.ldexp(sp, shift[:, None]).astype(np.float32)
        planes = [np.ldexp(x, shift[1:, None]).astype(np.float32) for x in (fm, fi, fd)]
    rec = np.zeros((len(sp), 6), np.uint32)
    rec[:, :5] = sp32.view(np.uint32)
    rec[:, 5] = e.astype(np.int32).view(np.uint32)
    return (*planes, rec)


def sample(model, planes, Lc, seq, i_from, i_to, j, seed=SEED):
    """msv.spl_sample on (fM, fI, fD, records) -> (segments, domains, ops, truncated)."""
    return msv.spl_sample(*planes, model[2], model[3], Lc=Lc, seq=seq, i_from=i_from, i_to=i_to, sample=j, seed=seed)


def cpu_ensemble(model, codes, Lc, seq, i_from, n_samples, seed=SEED):
    """The CPU twin of one item: the float64 matrix rounded once, then n_samples of the definition.  Returns
    (segments of all samples, list of (segments, domains, ops) per sample, planes)."""
    st, _, *mat = cpu_forward(model, codes, Lc)
    assert st == 0
    planes = as_float32(*mat)
    per, segs = [], []
    for j in range(n_samples):
        s, d, o, trunc = sample(model, planes, Lc, seq, i_from, i_from + len(codes) - 1, j, seed)
        assert not trunc
        per.append((s, d, o))
        segs.append(s)
    return np.concatenate(segs) if segs else np.zeros(0, _native.SEGMENT_DTYPE), per, planes


# ---- the batches --------------------------------------------------------------------------------------------------

FLANK, CORE = 12, 40
DRAWS = ("C<-E", "J<-E", "J loop", "M<-B")


def near(model, first: int, last: int, target: float) -> np.ndarray:
    """The residue of each state first .. last whose match score is nearest `target` nats: at 0 it changes little
    whether the residue is aligned or not, a little above 0 the row's E still grows."""
    return np.argmin(np.abs(model[0][:, first:last + 1] - target), axis=0).astype(np.uint8)


def copies_batch(model, target=0.0, fuzz=6, seed=910):
    """Sequence 0: two copies of the consensus of nodes 1 .. CORE back to back, no linker, between uniform flanks of
    FLANK; the last `fuzz` residues of the first copy and the first `fuzz` of the second are the ones `near` target,
    so where one domain ends and the next begins is spread over several residues (a sharp end closes the region by
    itself: end = occ there).  Sequence 1: the single-copy control.  Returns ((codes, offsets), [(first, last) of each
    planted copy in sequence 0], [(first, last) of each copy's core: the copy without its fuzzy residues])."""
    rng = np.random.Generator(np.random.PCG64(seed))
    fl = [rng.integers(0, 20, size=FLANK, dtype=np.uint8) for _ in range(4)]
    c1, c2 = consensus(model, 1, CORE).copy(), consensus(model, 1, CORE).copy()
    c1[CORE - fuzz:] = near(model, CORE - fuzz + 1, CORE, target)
    c2[:fuzz] = near(model, 1, fuzz, target)
    two = np.concatenate([fl[0], c1, c2, fl[1]])
    one = np.concatenate([fl[2], consensus(model, 1, CORE), fl[3]])
    a = FLANK + 1
    planted = [(a, a + CORE - 1), (a + CORE, a + 2 * CORE - 1)]
    cores = [(a, a + CORE - fuzz - 1), (a + CORE + fuzz, a + 2 * CORE - 1)]
    return _csr([two, one]), planted, cores


def rescale_sequence(model, seed, copies=8, fuzz=6):
    """A strong homolog: `copies` copies of the consensus of nodes 1 .. c (c drawn from 28 .. 44) back to back between
    flanks, the residues around every junction and at the last end scoring near log 2.  Each copy adds about 32 bits,
    so the exponent rises about once a copy, at a row that `seed` moves; the mild residues keep E growing through the
    junctions, where the samples disagree about J <- E, the J loop and M <- B (and, at the last end, about C <- E)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    parts = [rng.integers(0, 20, size=FLANK, dtype=np.uint8)]
    for c in range(copies):
        core = int(rng.integers(28, 45))
        x = consensus(model, 1, core).copy()
        if c > 0:
            x[:fuzz] = near(model, 1, fuzz, float(np.log(2.0)))
        x[core - fuzz:] = near(model, core - fuzz + 1, core, float(np.log(2.0)))
        parts.append(x)
    parts.append(rng.integers(0, 20, size=FLANK, dtype=np.uint8))
    return np.concatenate(parts)


def draws_on_rescaled_rows(records, samples, i0: int = 1):
    """{draw: the samples (of `samples`, each a segment array) that take it on a row whose recorded exponent differs
    from the row before}, for the four special draws."""
    expo = np.asarray(records)[:, 5].view(np.int32)
    changed = {int(i) for i in np.flatnonzero(np.diff(expo)) + 1}
    met = {k: 0 for k in DRAWS}
    for segs in samples:
        for k, rows in special_draws(segs, i0).items():
            met[k] += 1 if set(rows) & changed else 0
    return met


# The models of tests/test_gpu_split.py's capacity and layout tests, and for each the parameters of its two batches:
# (S, insert odds, which) -> (copies_batch's target, fuzz; rescale_sequence's seed).  They were searched on the CPU
# twin alone (the first of a fixed list of junctions, the first seed, for which every property below holds);
# tests/test_split_batches.py shows for every entry that the twin has the properties.  LENG 1 (S = 2, which = 2) has
# no room for a copy and has no entry.
PLAN = {
    (2, False, 0): (0.35, 8, 1),
    (2, False, 1): (0.35, 8, 58),
    (2, True, 0): (0.35, 8, 1),
    (2, True, 1): (0.35, 8, 210),
    (6, False, 0): (0.35, 8, 0),
    (6, False, 1): (0.35, 8, 36),
    (6, False, 2): (0.7, 8, 227),
    (6, True, 0): (0.35, 8, 51),
    (6, True, 1): (0.35, 8, 351),
    (6, True, 2): (0.7, 8, 220),
    (12, False, 0): (0.35, 8, 1),
    (12, False, 1): (0.0, 8, 147),
    (12, False, 2): (0.7, 8, 70),
    (12, True, 0): (0.35, 8, 1),
    (12, True, 1): (0.35, 8, 9),
    (12, True, 2): (0.7, 8, 6),
    (22, False, 0): (0.35, 8, 324),
    (22, False, 1): (0.35, 8, 113),
    (22, False, 2): (0.7, 8, 25),
    (22, True, 0): (0.35, 8, 161),
    (22, True, 1): (0.0, 8, 691),
    (22, True, 2): (0.7, 8, 80),
    (38, False, 0): (0.35, 8, 220),
    (38, False, 1): (0.0, 8, 114),
    (38, False, 2): (0.7, 8, 89),
    (38, True, 0): (0.35, 8, 84),
    (38, True, 1): (0.35, 8, 30),
    (38, True, 2): (0.7, 8, 121),
}


def gpu_model(S: int, inserts: bool, which: int):
    """which = 0, 1, 2: LENG 64 S, 64 S - 1, 64 (S - 2) + 1."""
    return base_model((64 * S, 64 * S - 1, 64 * (S - 2) + 1)[which], 31 + which, inserts)


def gpu_batches(S: int, inserts: bool, which: int):
    """(model, copies_batch's result, the strong homolog) of one PLAN entry."""
    target, fuzz, seed = PLAN[(S, inserts, which)]
    model = gpu_model(S, inserts, which)
    return model, copies_batch(model, target, fuzz), rescale_sequence(model, seed)


def special_draws(segments, i0: int = 1):
    """The special-state draws a sample's segments imply, as rows relative to the envelope (i0 = the envelope's
    i_from): {"C<-E": [i], "J<-E": [i, ..], "J loop": [i, ..], "M<-B": [i, ..]} -- row i is the NEWER row of the
    draw (C(i), J(i), M(i, k))."""
    out = {"C<-E": [], "J<-E": [], "J loop": [], "M<-B": []}
    segs = [(int(g["i_from"]) - i0 + 1, int(g["i_to"]) - i0 + 1) for g in segments]
    for d, (a, b) in enumerate(segs):
        out["M<-B"].append(a)
        if d + 1 < len(segs):
            out["J<-E"].append(b)
            out["J loop"] += list(range(b + 1, segs[d + 1][0]))
        else:
            out["C<-E"].append(b)
    return out


# ---- the device, on a raw msv_dom_profile (decode_lib.create_profile) ---------------------------------------------

def gpu_sample(p, M, codes, offsets, items, n_samples, seed=SEED, workspace_bytes=0, keep=False, stream=None):
    """msv_spl_sample_batch on a raw profile -> (status, dict or None): env, sample_off, segments, stats and, with
    keep, mat[q] = (fM, fI, fD, records)."""
    codes = np.ascontiguousarray(codes, np.uint8)
    offsets = np.ascontiguousarray(offsets, np.uint64)
    it = np.zeros(len(items), _native.ITEM_DTYPE)
    for q, (s, a, b) in enumerate(items):
        it[q] = (s, a, b)
    L = _native.lib()
    r = C.c_void_p()
    opts = _native.SplOptions(workspace_bytes, seed, n_samples, 1 if keep else 0, stream)
    st = L.msv_spl_sample_batch(p, _ptr(codes), offsets.ctypes.data, len(offsets) - 1, _ptr(it), len(it),
                                C.byref(opts), C.byref(r))
    if not r.value:
        return st, None
    try:
        m = L.msv_spl_result_count(r)
        out = {"env": np.zeros(m, np.float32), "sample_off": np.zeros(m * n_samples + 1, np.uint64),
               "segments": np.zeros(L.msv_spl_result_segments(r), _native.SEGMENT_DTYPE)}
        assert L.msv_spl_result_copy(r, _ptr(out["env"]), out["sample_off"].ctypes.data, _ptr(out["segments"])) == 0
        stats = _native.SplStats()
        assert L.msv_spl_result_stats(r, C.byref(stats)) == 0
        out["stats"] = {f: getattr(stats, f) for f, _ in stats._fields_}
        if keep and st in (0, 4):
            out["mat"] = []
            for q in range(m):
                Le = int(it["i_to"][q]) - int(it["i_from"][q]) + 1
                fm, fi, fd = (np.zeros((Le, M), np.float32) for _ in range(3))
                rec = np.zeros((Le + 1, 6), np.uint32)
                assert L.msv_spl_result_matrix(r, q, _ptr(fm), _ptr(fi), _ptr(fd), rec.ctypes.data) == 0
                out["mat"].append((fm, fi, fd, rec))
    finally:
        L.msv_spl_result_free(r)
    return st, out


def item_segments(out, q, n_samples):
    """The bytes of item q's samples: (segment counts per sample, segments)."""
    off = out["sample_off"][q * n_samples:(q + 1) * n_samples + 1].astype(np.int64)
    return np.diff(off), out["segments"][off[0]:off[-1]]


def sample_counts(model, planes, Lc, seq, i_from, i_to, n_samples, seed=SEED):
    """n_samples of msv_spl_sample on one set of planes, one call a sample into buffers sized for the longest path:
    ({align_lib.path_key: count}, truncated samples)."""
    from align_lib import path_key
    msc, isc, tsc, consts = model
    fm, fi, fd, rec = (np.ascontiguousarray(x) for x in planes)
    tsc = np.ascontiguousarray(tsc, np.float32)
    Le, M = i_to - i_from + 1, tsc.shape[0]
    cap_d, cap_o = Le + 1, Le * (M + 1) + 1
    segs = np.zeros(cap_d, _native.SEGMENT_DTYPE)
    doms = np.zeros(cap_d, _native.DOMAIN_DTYPE)
    ops = np.zeros(cap_o, np.uint8)
    fn = _native.lib().msv_spl_sample
    ns, no, tr = C.c_uint32(), C.c_uint64(), C.c_int()
    head = (fm.ctypes.data, fi.ctypes.data, fd.ctypes.data, rec.ctypes.data, tsc.ctypes.data, M,
            *[float(x) for x in consts], Lc, seed, seq, i_from, i_to)
    tail = (C.byref(ns), C.byref(no), C.byref(tr), segs.ctypes.data, doms.ctypes.data, ops.ctypes.data)
    raw, truncated = {}, 0
    for j in range(n_samples):
        ns.value, no.value = cap_d, cap_o
        assert fn(*head, j, *tail) == 0
        truncated += tr.value
        key = (ns.value, doms[:ns.value].tobytes(), ops[:no.value].tobytes())
        raw[key] = raw.get(key, 0) + 1
    out = {}
    for (nd, d, o), count in raw.items():
        key = path_key(np.frombuffer(d, np.dtype(_native.DOMAIN_DTYPE), count=nd), np.frombuffer(o, np.uint8))
        out[key] = out.get(key, 0) + count
    return out, truncated


def host_segments(model, mat, Lc, seq, i_from, i_to, n_samples, seed=SEED):
    """THE definition on one item's (downloaded) matrix, every sample: (segment counts per sample, segments,
    truncated samples) -- what item_segments gives for the device."""
    fm, fi, fd, rec = (np.ascontiguousarray(x) for x in mat)
    tsc = np.ascontiguousarray(model[2], np.float32)
    Le, M = i_to - i_from + 1, tsc.shape[0]
    cap = Le + 1
    segs = np.zeros(cap, _native.SEGMENT_DTYPE)
    fn = _native.lib().msv_spl_sample
    ns, no, tr = C.c_uint32(), C.c_uint64(), C.c_int()
    head = (fm.ctypes.data, fi.ctypes.data, fd.ctypes.data, rec.ctypes.data, tsc.ctypes.data, M,
            *[float(x) for x in model[3]], Lc, seed, seq, i_from, i_to)
    tail = (C.byref(ns), C.byref(no), C.byref(tr), segs.ctypes.data, None, None)
    counts, parts, truncated = np.zeros(n_samples, np.int64), [], 0
    for j in range(n_samples):
        ns.value, no.value = cap, 0
        assert fn(*head, j, *tail) == 0
        truncated += tr.value
        counts[j] = ns.value
        parts.append(segs[:ns.value].copy())
    return counts, np.concatenate(parts) if parts else segs[:0], truncated
