"""Shared by the bias filter's tests (test helper, not a conftest): the library's host functions through
the C-ABI over raw arrays, the model of msv.h's "Bias filter" block restated in numpy (an explicit sum over every
state path, the filtered P-values in float64), msv.h's tolerance, the synthetic compositions, and the batches the GPU
tests run -- built without a GPU, so that a CPU test can assert the cascade batch's premise on the float64 twin."""
import ctypes as C
import functools
import itertools
import os

import numpy as np

from hmm_fasta_viterbi_amd import _native
from hmm_fasta_viterbi_amd.synthetic import background_batch, concat_batches
from oracle_lib import OracleProfile, profile_path
from state_batches import _csr

U = 2.0 ** -24
LN2 = float(np.log(2.0))
GUMBEL, EXPONENTIAL = _native.BF_GUMBEL, _native.BF_EXPONENTIAL
CHUNK, TRIP = 16, 1024  # a lane's residues per trip and a wave's (msv_bf_info reports them; the GPU tests assert it)
LENGTHS = [0, 1, 2, 15, 16, 17, 63 * 16, 1023, 1024, 1025, 2047, 2048, 2049, 20000]


def _ptr(a):
    return a.ctypes.data if a.size else None


def background():
    return np.ctypeslib.as_array(_native.lib().msv_background_frequencies(), (20,)).copy()


def numpy_compo(path):
    """The COMPO line of a profile file, parsed in numpy: float32(exp(-float32(value)))."""
    for line in open(path):
        w = line.split()
        if w and w[0] == "COMPO":
            v = np.array([np.float32(x) for x in w[1:21]], np.float32)
            return np.exp(-v.astype(np.float64)).astype(np.float32)
    raise ValueError("no COMPO line")


def file_compo(name):
    """(compo float32 [20], model_length = LENG + 1) of a bundled profile, by the library's parser."""
    L = _native.lib()
    h = C.c_void_p()
    assert L.msv_hmm_read(profile_path(name).encode(), C.byref(h)) == 0
    try:
        return np.ctypeslib.as_array(L.msv_hmm_compo(h), (20,)).copy(), int(L.msv_hmm_model_length(h))
    finally:
        L.msv_hmm_destroy(h)


def synthetic_compo(seed, lo, hi):
    """A composition whose odds against the background spread log-uniformly over [lo, hi] before it is renormalised
    (the two ends are both present)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    f = background().astype(np.float64)
    r = np.exp(rng.uniform(np.log(lo), np.log(hi), 20))
    r[rng.permutation(20)[:2]] = lo, hi
    c = f * r
    return (c / c.sum()).astype(np.float32)


def odds(compo, bg):
    return compo.astype(np.float64) / bg.astype(np.float64)


def cpu_score(compo, bg, model_length, codes):
    """msv_bf_cpu_score -> (status, float64)."""
    compo, bg = np.ascontiguousarray(compo, np.float32), np.ascontiguousarray(bg, np.float32)
    c = np.ascontiguousarray(codes, np.uint8)
    out = C.c_double(-1.0)
    st = _native.lib().msv_bf_cpu_score(compo.ctypes.data, bg.ctypes.data, model_length, _ptr(c), len(c), C.byref(out))
    return st, out.value


def cpu_score_batch(compo, bg, model_length, codes, offsets):
    compo, bg = np.ascontiguousarray(compo, np.float32), np.ascontiguousarray(bg, np.float32)
    codes, offsets = np.ascontiguousarray(codes, np.uint8), np.ascontiguousarray(offsets, np.uint64)
    out = np.zeros(len(offsets) - 1)
    st = _native.lib().msv_bf_cpu_score_batch(compo.ctypes.data, bg.ctypes.data, model_length, _ptr(codes),
                                              offsets.ctypes.data, len(out), out.ctypes.data)
    return st, out


def pvalues(scores, bias, offsets, location, scale, kind):
    """msv_bf_pvalues -> (status, float64 [n])."""
    scores, bias = np.ascontiguousarray(scores, np.float32), np.ascontiguousarray(bias, np.float32)
    offsets = np.ascontiguousarray(offsets, np.uint64)
    out = np.zeros(len(offsets) - 1)
    st = _native.lib().msv_bf_pvalues(_ptr(scores), _ptr(bias), offsets.ctypes.data, len(out), location, scale, kind,
                                      _ptr(out))
    return st, out


def transitions(model_length):
    """(T [2][2], pi [2]) in float64, L1 = LENG / 8 as a float."""
    L0, L1 = 400.0, float(np.float32(model_length - 1) / np.float32(8.0))
    T = np.array([[L0 / (L0 + 1.0), 1.0 / (L0 + 1.0)], [1.0 / (L1 + 1.0), L1 / (L1 + 1.0)]])
    return T, np.array([0.999, 0.001])


def path_sum(compo, bg, model_length, codes):
    """log of the summed odds of all 2^L state paths, each path's product formed on its own."""
    T, pi = transitions(model_length)
    r = odds(compo, bg)
    total = 0.0
    for path in itertools.product((0, 1), repeat=len(codes)):
        p = pi[path[0]]
        for i, s in enumerate(path):
            if i:
                p *= T[path[i - 1], s]
            if s:
                p *= r[codes[i]]
        total += p
    return float(np.log(total))


def null1(L):
    """msv_pvalues' null1 score, float32 as the library rounds it."""
    p1 = np.float32(L) / np.float32(L + 1)
    return np.float32(float(L) * np.log(float(p1)) + np.log(1.0 - float(p1)))


def pvalue64(score, bias, L, location, scale, kind):
    """The filtered P-value restated: the bit score in float32, as msv.h defines it (msv_pvalues' nullsc and bits are
    floats), the tail in float64."""
    if L == 0:
        return 1.0
    with np.errstate(invalid="ignore"):
        bits = float((np.float32(score) - null1(L) - np.float32(bias)) / np.float32(0.69314718055994529))
    if kind == GUMBEL:
        return float(-np.expm1(-np.exp(-float(scale) * (bits - float(location)))))
    return 1.0 if bits < location else float(np.exp(-float(scale) * (bits - float(location))))


def tolerance(lengths, cpu):
    """msv.h: |gpu - cpu| <= k u / (1 - k u) + u |cpu|, k = 5 L + 14 ceil(L / 1024) + 4."""
    L = np.asarray(lengths, np.float64)
    k = 5.0 * L + 14.0 * np.ceil(L / TRIP) + 4.0
    return k * U / (1.0 - k * U) + U * np.abs(np.asarray(cpu, np.float64))


# ---- the GPU tests' inputs ------------------------------------------------------------------------------------------

def models():
    """name -> (compo, background, model_length): two bundled profiles, LENG 1 and an extreme composition."""
    bg = background()
    out = {}
    for name in ("100", "2405"):
        compo, M = file_compo(name)
        out[name] = (compo, bg, M)
    out["leng1"] = (synthetic_compo(11, 0.5, 2.0), bg, 2)
    out["extreme"] = (synthetic_compo(12, 0.05, 20.0), bg, 301)
    return out


def length_batches(compo, bg, seed):
    """The LENGTHS batch three times: random residues, and homopolymers of the residues with the largest and the
    smallest odds."""
    rng = np.random.Generator(np.random.PCG64(seed))
    r = odds(compo, bg)
    rand = [rng.integers(0, 20, L).astype(np.uint8) for L in LENGTHS]
    hi = [np.full(L, int(np.argmax(r)), np.uint8) for L in LENGTHS]
    lo = [np.full(L, int(np.argmin(r)), np.uint8) for L in LENGTHS]
    return {"random": _csr(rand), "largest_r": _csr(hi), "smallest_r": _csr(lo)}


CASCADE_SEED = 3
N_BACKGROUND, N_PLANTED, CASCADE_LENGTH = 300, 30, 400


@functools.lru_cache(maxsize=None)
def cascade_batch(seed=CASCADE_SEED):
    """300 background sequences of length 400, then 30 low-complexity ones: background sequences into which runs of
    the three residues with the largest odds of 100.hmm's composition are planted."""
    compo, _ = file_compo("100")
    top = np.argsort(-odds(compo, background()))[:3]
    bgc, bgo = background_batch(seed, N_BACKGROUND, CASCADE_LENGTH)
    pc, po = background_batch(seed + 1000, N_PLANTED, CASCADE_LENGTH)
    rng = np.random.Generator(np.random.PCG64(seed + 2000))
    pc = pc.copy()
    for q in range(N_PLANTED):
        lo = int(po[q])
        # a growing share of the sequence in runs of 5 .. 40 of one of the three residues
        share = (q + 1) / N_PLANTED
        pos = 0
        while pos < CASCADE_LENGTH:
            run = int(rng.integers(5, 41))
            if rng.random() < share:
                pc[lo + pos:lo + min(pos + run, CASCADE_LENGTH)] = top[int(rng.integers(0, 3))]
            pos += run
    return concat_batches((bgc, bgo), (pc, po))


@functools.lru_cache(maxsize=None)
def cascade_reference(seed=CASCADE_SEED):
    """Of cascade_batch on 100.hmm, on the CPU: (msv scores float32 by the oracle, bias float64 by the twin, the MSV
    bits against null1, the filtered bits, the bits at which P = F1 = 0.02)."""
    codes, offsets = cascade_batch(seed)
    o = OracleProfile("100")
    msc = o.score_batch(codes, offsets)
    compo, M = file_compo("100")
    st, bias = cpu_score_batch(compo, background(), M, codes, offsets)
    assert st == 0
    mu, lam = o.stats()[0], o.stats()[1]
    n1 = np.array([float(null1(int(L))) for L in np.diff(offsets)])
    bits1 = (msc.astype(np.float64) - n1) / LN2
    bits2 = bits1 - bias / LN2
    # P = 1 - exp(-exp(-lam (b - mu))) = F1
    cut = float(mu) - np.log(-np.log1p(-0.02)) / float(lam)
    return msc, bias, bits1, bits2, cut
