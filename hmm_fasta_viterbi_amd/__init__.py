"""hmm_fasta_viterbi_amd -- MI355X-native MSV (Multiple Segment Viterbi) scoring engine.

Python mirror of the reference's C++ class surface, bound to libmsv_hip.so (include/msv.h):

    Profile_HMM(path)                       data_readers/Profile_HMM.hpp:21-49
    FASTA_protein_sequences(path)           data_readers/FASTA_protein_sequences.hpp:9-14
    MSV_HMM(profile).run_on_sequence(seq)   algorithms/MSV_HMM.hpp:17-44
                    .parallel_run_on_sequence(seq, should_specialize=False)
                    .score_batch(...)       (new: one fused kernel launch per batch)
    Viterbi_HMM(profile)                    (new, SURVEY 8(f)-4: the Viterbi stage over the parse the
                                             reference never scores with, Profile_HMM.cpp:107-120)
    filter_pipeline(msv, vit, ...)          MSV -> P-value -> F1 -> Viterbi on the survivors, on the GPU
    Forward_HMM(profile)                    (new, DESIGN 4.9: the summed odds of every alignment, with P-values)
    search_pipeline(msv, vit, fwd, ...)     MSV -> F1 -> Viterbi -> F2 -> Forward -> P-value, on the GPU
    Domain_HMM(profile)                     (new, DESIGN 4.10: Backward, domain posteriors and envelopes of each hit;
                                             DESIGN 4.11: align_batch, the posterior decoding and optimal-accuracy
                                             alignment of each envelope)
    calibrate(profile, msv, vit, fwd)       (new, DESIGN 4.15: the engines' own mu, tau and lambda, fitted on the GPU;
                                             search_pipeline(..., stats=) takes them in place of the file's)
    Emitter(profile).emit(n)                (new, DESIGN 4.16: sequences drawn from the profile on the GPU, with the
                                             true domains and ops of each as a Traces)

Sequences use the reference's form ('#' sentinel + one-letter residues) or packed codes
0..19 (alphabetical A C D E F G H I K L M N P Q R S T V W Y) with CSR offsets.
Every score is computed by the hand-written gfx950 kernel; there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import Iterable, Sequence

import numpy as np

from . import _native
from ._native import MSVError, check

__all__ = [
    "AMINO_ACIDS", "MSVError", "Profile_HMM", "FASTA_protein_sequences", "MSV_HMM", "pack_sequences",
    "encode", "sequence_transitions", "device_count", "score_grid", "score_grid_device", "score_batch_multi",
    "shard_bounds", "FASTA_device", "MultiGPU", "Viterbi_HMM", "filter_pipeline", "INSERTS_ZERO",
    "INSERTS_LOG_ODDS", "Traces", "Forward_HMM", "search_pipeline", "Domain_HMM", "Envelopes", "dom_regions",
    "Alignments", "aln_oa", "Bias_filter", "background_frequencies", "Ensembles", "dom_is_multidomain", "spl_cluster",
    "spl_sample", "Calibration", "calibrate", "cal_cpu_calibrate", "cal_lambda", "cal_thresholds",
    "cal_codes_of_draws", "cal_generate", "cal_fit_location", "cal_fit_gumbel", "cal_tau", "write_hmm_stats",
    "Emitter", "Emitted", "emit_generate", "emit_path_score", "emit_tables",
]

INSERTS_ZERO = 0      # HMMER3's insert scores (background emissions: 0)
INSERTS_LOG_ODDS = 1  # logf(insert_emissions / background) of the reference's parse

AMINO_ACIDS = "ACDEFGHIKLMNPQRSTVWY"  # MSV_HMM.cpp:29-31
_LUT = np.full(256, 254, np.uint8)
for _i, _c in enumerate(AMINO_ACIDS):
    _LUT[ord(_c)] = _i
_LUT[ord("#")] = 255


def _loaded_lib():
    """The loaded library, or None (also during interpreter shutdown, when module globals such as
    `_native` may already be cleared before the last destructor runs)."""
    native = globals().get("_native")
    return getattr(native, "_lib", None) if native is not None else None


def device_count() -> int:
    n = C.c_int(0)
    _native.lib().msv_device_count(C.byref(n))
    return n.value


class _HostBuffer:
    """Owner of one msv_host_alloc block; freed when the last numpy view of it goes away."""

    def __init__(self, nbytes: int):
        self.ptr = C.c_void_p()
        check(_native.lib().msv_host_alloc(max(int(nbytes), 1), C.byref(self.ptr)), "msv_host_alloc")
        self.nbytes = int(nbytes)

    def __del__(self):
        lib = _loaded_lib()
        if lib is not None and self.ptr:
            lib.msv_host_free(self.ptr)
            self.ptr = C.c_void_p()


def pinned_empty(shape, dtype=np.uint8) -> np.ndarray:
    """A numpy array in page-locked host memory (msv_host_alloc).  score_batch reads residues from such
    an array in place on the GPU (no staging copy) and writes scores into one directly."""
    dt = np.dtype(dtype)
    count = int(np.prod(shape)) if np.ndim(shape) else int(shape)
    owner = _HostBuffer(count * dt.itemsize)
    raw = (C.c_uint8 * max(owner.nbytes, 1)).from_address(owner.ptr.value)
    raw.owner = owner  # every view keeps `raw` (its base), `raw` keeps the allocation
    return np.frombuffer(raw, dtype=dt, count=count).reshape(shape)


def sequence_transitions(L: int) -> tuple[float, float]:
    """(tr_loop, tr_move) of MSV_HMM::init_transitions_depend_on_seq (MSV_HMM.cpp:59-64)."""
    a, b = C.c_float(), C.c_float()
    _native.lib().msv_sequence_transitions(L, C.byref(a), C.byref(b))
    return a.value, b.value


def encode(residues: str) -> np.ndarray:
    """One-letter residues (no '#') -> codes 0..19; IndexError on anything else (the
    reference's amino_acid_num.at throws std::out_of_range, MSV_HMM.cpp:101)."""
    codes = _LUT[np.frombuffer(residues.encode("latin-1"), np.uint8)]
    if codes.size and codes.max() >= 20:
        raise IndexError("residue outside the 20 amino acids")
    return codes


def pack_sequences(seqs: Sequence[str]) -> tuple[np.ndarray, np.ndarray]:
    """'#'-prefixed sequences -> (codes uint8, offsets uint64[n+1])."""
    lens = np.fromiter((max(len(s) - 1, 0) for s in seqs), np.uint64, count=len(seqs))
    offsets = np.zeros(len(seqs) + 1, np.uint64)
    np.cumsum(lens, out=offsets[1:])
    body = "".join(s[1:] for s in seqs)
    return encode(body), offsets


def _batch(seqs, codes, offsets) -> tuple[np.ndarray, np.ndarray, int]:
    """A host batch as the C-ABI takes it: (codes uint8, offsets uint64[n+1], n), both contiguous; `seqs`
    ('#'-prefixed strings), when given, are packed into them."""
    if seqs is not None:
        codes, offsets = pack_sequences(seqs)
    codes = np.ascontiguousarray(codes, np.uint8)
    offsets = np.ascontiguousarray(offsets, np.uint64)
    return codes, offsets, len(offsets) - 1


def _ptr(a: np.ndarray):
    """The array's address, NULL for an empty one."""
    return a.ctypes.data if a.size else None


def _check_residues(status: int, what: str = "") -> None:
    """check(), with a residue outside the 20 as the reference's IndexError (amino_acid_num.at, MSV_HMM.cpp:101)."""
    if status == _native.MSV_ERR_BAD_RESIDUE:
        raise IndexError("residue outside the 20 amino acids")
    check(status, what)


def _pvalues(fn: str, scores: np.ndarray, offsets: np.ndarray, location: float, scale: float) -> np.ndarray:
    """Host P-values (msv_pvalues / msv_fwd_pvalues) of n scores, lengths from the offsets -> float64 [n]."""
    scores = np.ascontiguousarray(scores, np.float32)
    offsets = np.ascontiguousarray(offsets, np.uint64)
    n = len(offsets) - 1
    if scores.shape != (n,):
        raise ValueError("scores and offsets disagree")
    out = np.zeros(n, np.float64)
    check(getattr(_native.lib(), fn)(scores.ctypes.data, offsets.ctypes.data, n, location, scale, out.ctypes.data), fn)
    return out


class Profile_HMM:
    """Parsed HMMER3 profile (C++ parser in libmsv_hip.so, Profile_HMM.cpp:48-60 semantics)."""

    def __init__(self, file_path: str):
        L = _native.lib()
        h = C.c_void_p()
        check(L.msv_hmm_read(str(file_path).encode(), C.byref(h)), f"Profile_HMM({file_path})")
        self._h = h
        self.path = str(file_path)
        self.model_length = int(L.msv_hmm_model_length(h))
        self.name = L.msv_hmm_name(h).decode("latin-1")
        st = (C.c_float * 6)()
        L.msv_hmm_stats(h, st)
        (self.stats_local_msv_mu, self.stats_local_msv_lambda, self.stats_local_viterbi_mu,
         self.stats_local_viterbi_lambda, self.stats_local_forward_theta,
         self.stats_local_forward_lambda) = [float(np.float32(x)) for x in st]
        M = self.model_length
        self.match_emissions = np.ctypeslib.as_array(L.msv_hmm_match_emissions(h), (M, 20)).copy()
        self.insert_emissions = np.ctypeslib.as_array(L.msv_hmm_insert_emissions(h), (M, 20)).copy()
        self.transitions = np.ctypeslib.as_array(L.msv_hmm_transitions(h), (M, 7)).copy()
        # the COMPO line: the model's average composition (the bias filter's second state emits it)
        self.compo = np.ctypeslib.as_array(L.msv_hmm_compo(h), (20,)).copy()

    def msv_scores(self) -> tuple[np.ndarray, float, float, float]:
        """MSV host precompute (MSV_HMM.cpp:35-57): ([20, M] log-odds, tr_B_Mk, tr_E_C, tr_E_J)."""
        es = np.zeros((20, self.model_length), np.float32)
        b, c, j = C.c_float(), C.c_float(), C.c_float()
        check(_native.lib().msv_hmm_msv_scores(self._h, es.ctypes.data_as(C.POINTER(C.c_float)), C.byref(b),
                                                C.byref(c), C.byref(j)))
        return es, b.value, c.value, j.value

    def __del__(self):
        lib = _loaded_lib()
        if getattr(self, "_h", None) and lib is not None:
            lib.msv_hmm_destroy(self._h)
            self._h = None


class FASTA_protein_sequences:
    """FASTA reader (FASTA_protein_sequences.cpp:9-44 semantics), packed straight to codes."""

    def __init__(self, file_path: str):
        L = _native.lib()
        f = C.c_void_p()
        check(L.msv_fasta_read(str(file_path).encode(), C.byref(f)), f"FASTA_protein_sequences({file_path})")
        try:
            n = int(L.msv_fasta_count(f))
            self.offsets = np.ctypeslib.as_array(L.msv_fasta_offsets(f), (n + 1,)).copy()
            total = int(self.offsets[-1])
            self.codes = (np.ctypeslib.as_array(L.msv_fasta_codes(f), (total,)).copy() if total
                          else np.zeros(0, np.uint8))
            self.headers = [L.msv_fasta_header(f, i).decode("latin-1") for i in range(n)]
            self.rejected = int(L.msv_fasta_rejected(f))
        finally:
            L.msv_fasta_destroy(f)
        self._sequences = None

    @property
    def sequences(self) -> list[str]:
        """'#'-prefixed residue strings (FASTA_protein_sequences.cpp:19-20), built on first use; the
        packed `codes`/`offsets` are what the scorer consumes."""
        if self._sequences is None:
            letters = np.frombuffer((AMINO_ACIDS + "#").encode(), np.uint8)
            text = letters[np.minimum(self.codes, 20)].tobytes().decode()
            offs = self.offsets.tolist()
            self._sequences = ["#" + text[offs[i]:offs[i + 1]] for i in range(len(offs) - 1)]
        return self._sequences

    def __len__(self):
        return len(self.offsets) - 1


class MSV_HMM:
    """MSV scorer for one profile on one GPU (MSV_HMM.hpp:17-44); every score comes from the
    fused gfx950 kernel.  Not thread-safe per instance, like the reference."""

    def __init__(self, base_hmm: Profile_HMM, device: int = 0):
        L = _native.lib()
        self.model_length = base_hmm.model_length
        self.emission_scores, self.tr_B_Mk, self.tr_E_C, self.tr_E_J = base_hmm.msv_scores()
        p = C.c_void_p()
        es = np.ascontiguousarray(self.emission_scores)
        check(L.msv_profile_create(device, es.ctypes.data, self.model_length, self.tr_B_Mk, self.tr_E_C,
                                   self.tr_E_J, C.byref(p)), "msv_profile_create")
        self._p = p
        self._inflight = {}  # msv_score_batch_async tickets -> the arrays the device still reads/writes
        self.device = device
        # STATS LOCAL MSV (Profile_HMM.cpp:83-85): parsed by the reference, used here for P-values
        self.msv_mu = base_hmm.stats_local_msv_mu
        self.msv_lambda = base_hmm.stats_local_msv_lambda

    # -- reference surface ------------------------------------------------------------------
    def run_on_sequence(self, seq: str) -> float:
        return float(self.score_batch([seq])[0])

    def parallel_run_on_sequence(self, seq: str, should_specialize: bool = False) -> float:
        # should_specialize (JIT -D constants, MSV_HMM.cpp:322-337) is always on here: the kernel
        # is a compile-time specialisation on (G, S); both settings return the same score.
        return self.run_on_sequence(seq)

    # -- batch API --------------------------------------------------------------------------
    def score_batch(self, seqs: Sequence[str] | None = None, *, codes: np.ndarray | None = None,
                    offsets: np.ndarray | None = None, out: np.ndarray | None = None) -> np.ndarray:
        """Scores of a host batch (msv_score_batch).  Page-locked `codes` (msv.pinned_empty, torch
        pin_memory().numpy()) are read by the kernel in place, with no staging copy; a page-locked `out`
        (float32[n]) is written by the kernel directly."""
        codes, offsets, n = _batch(seqs, codes, offsets)
        if out is None:
            out = np.zeros(n, np.float32)
        elif out.dtype != np.float32 or out.shape != (n,) or not out.flags.c_contiguous:
            raise ValueError("out must be a contiguous float32 array of n scores")
        _check_residues(_native.lib().msv_score_batch(self._p, _ptr(codes), offsets.ctypes.data, n, out.ctypes.data,
                                                      None), "msv_score_batch")
        return out

    def score_batch_async(self, codes: np.ndarray, offsets: np.ndarray, out: np.ndarray | None = None) -> int:
        """Enqueue a host batch (msv_score_batch_async) and return a ticket; `wait(ticket)` returns
        the scores.  At most three calls outstanding; pinned arrays (torch pin_memory().numpy()) make
        the copies overlap the previous call's kernel.  The arrays are held until the wait."""
        codes, offsets, n = _batch(None, codes, offsets)
        if out is None:
            out = np.zeros(n, np.float32)
        if out.dtype != np.float32 or out.shape != (n,) or not out.flags.c_contiguous:
            raise ValueError("out must be a contiguous float32 array of n scores")
        t = C.c_uint64(0)
        check(_native.lib().msv_score_batch_async(self._p, _ptr(codes), offsets.ctypes.data, n, out.ctypes.data,
                                                  C.byref(t)), "msv_score_batch_async")
        self._inflight[t.value] = (codes, offsets, out)
        return t.value

    def wait(self, ticket: int) -> np.ndarray:
        """Scores of an msv_score_batch_async call (raises its kernel-latched errors)."""
        st = _native.lib().msv_profile_wait(self._p, ticket)
        _, _, out = self._inflight.pop(ticket, (None, None, None))
        _check_residues(st, "msv_profile_wait")
        return out

    def score_batch_device(self, residues_ptr: int, residues_len: int, offsets_ptr: int, n: int, scores_ptr: int,
                           order_ptr: int | None = None, stream: int | None = None) -> None:
        """Device-resident batch (raw device pointers, e.g. torch tensor .data_ptr()); async on
        `stream` (a hipStream_t handle, e.g. torch.cuda.current_stream().cuda_stream)."""
        check(_native.lib().msv_score_batch_device(self._p, residues_ptr, residues_len, offsets_ptr, n, order_ptr,
                                                   scores_ptr, stream), "msv_score_batch_device")

    def order_longest_first(self, offsets_ptr: int, n: int, order_ptr: int, stream: int | None = None) -> None:
        check(_native.lib().msv_order_longest_first(self._p, offsets_ptr, n, order_ptr, stream))

    def bind_stream(self, stream: int | None) -> None:
        """Declare `stream` (a hipStream_t handle that outlives the binding) as this profile's working
        stream: its launches skip the per-launch slot event (msv_profile_bind_stream).  None unbinds."""
        check(_native.lib().msv_profile_bind_stream(self._p, stream), "msv_profile_bind_stream")

    def check(self, stream: int | None = None) -> None:
        _check_residues(_native.lib().msv_profile_check(self._p, stream), "msv_profile_check")

    def reserve_length(self, max_length: int) -> None:
        check(_native.lib().msv_profile_reserve_length(self._p, max_length))

    # -- MSV filter stage (HMMER3 formula, parity unpinned) --------------------
    def pvalues(self, scores: np.ndarray, offsets: np.ndarray) -> np.ndarray:
        """P-values of MSV scores against this profile's STATS LOCAL MSV Gumbel (msv.h)."""
        return _pvalues("msv_pvalues", scores, offsets, self.msv_mu, self.msv_lambda)

    def pvalues_device(self, scores_ptr: int, offsets_ptr: int, n: int, pvalues_ptr: int,
                       stream: int | None = None) -> None:
        """Device P-values (float64 out) for device scores/offsets, async on `stream`."""
        check(_native.lib().msv_pvalues_device(self.device, scores_ptr, offsets_ptr, n, self.msv_mu, self.msv_lambda,
                                               pvalues_ptr, stream), "msv_pvalues_device")

    def msv_filter(self, seqs: Sequence[str] | None = None, *, codes: np.ndarray | None = None,
                   offsets: np.ndarray | None = None, F1: float = 0.02, bias: "Bias_filter | None" = None,
                   stats=None):
        """Scores, P-values and the pass mask of HMMER3's MSV filter threshold (P <= F1, default
        0.02 as hmmsearch's --F1).  With bias=Bias_filter both of HMMER3's tests apply -- P <= F1 against null1,
        then P <= F1 with the bias filter's score (msv.h "Bias filter") -- and the call returns (scores, filtered
        P-values, mask, bias); the bias is 0 where the first test failed, so such a P-value is the null1 one.
        stats (a Calibration or six floats) replaces the file's STATS LOCAL MSV."""
        if seqs is not None:
            codes, offsets = pack_sequences(seqs)
        mu, lam = (self.msv_mu, self.msv_lambda) if stats is None else _six_stats(stats)[:2]
        sc = self.score_batch(codes=codes, offsets=offsets)
        pv = _pvalues("msv_pvalues", sc, offsets, mu, lam)
        if bias is None:
            return sc, pv, pv <= F1
        b = bias.score_batch(codes=codes, offsets=offsets, select=np.flatnonzero(pv <= F1))
        fpv = bias.pvalues(sc, b, offsets, mu, lam, kind="gumbel")
        return sc, fpv, fpv <= F1, b

    def score_fasta_device(self, fasta: "FASTA_device") -> np.ndarray:
        """Scores of a GPU-parsed FASTA set (msv_score_fasta_device): no host parse, no H2D of residues."""
        out = np.zeros(fasta.count, np.float32)
        _check_residues(_native.lib().msv_score_fasta_device(self._p, fasta._f, out.ctypes.data),
                        "msv_score_fasta_device")
        return out

    def set_variant(self, name: str) -> None:
        check(_native.lib().msv_profile_set_variant(self._p, name.encode()), f"set_variant({name})")

    @staticmethod
    def variants() -> list[str]:
        L = _native.lib()
        return [L.msv_variant_name(i).decode() for i in range(L.msv_variant_count())]

    def describe(self) -> dict:
        info = _native.KernelInfo()
        check(_native.lib().msv_profile_describe(self._p, C.byref(info)))
        return info.as_dict()

    def variant_for(self, n: int) -> str:
        """The kernel variant a batch of n sequences runs (latency / mid / throughput plan)."""
        return _native.lib().msv_profile_variant_for(self._p, n).decode()

    def close(self):
        lib = _loaded_lib()
        if getattr(self, "_p", None) and lib is not None:
            lib.msv_profile_destroy(self._p)
            self._p = None

    def __del__(self):
        self.close()


class Traces:
    """One optimal Viterbi state path per traced sequence (msv.h "Viterbi traces"): `scores` float32 [n],
    `domain_offsets` uint64 [n + 1] (entry q's domains are domains[domain_offsets[q]:domain_offsets[q + 1]]),
    `domains` a structured array (seq, i_from, i_to, k_from, k_to, ops_len, ops_begin) and `ops`, one byte
    'M' / 'I' / 'D' per core state visited.  `status` is the call's status name (MSV_OK, or the scoring calls'
    error when strict=False let a bad sequence through with no domains); `stats` what the device did."""

    def __init__(self, scores, domain_offsets, domains, ops, *, status="MSV_OK", stats=None, codes=None,
                 offsets=None, consensus=None):
        self.scores, self.domain_offsets, self.domains, self.ops = scores, domain_offsets, domains, ops
        self.status = status
        self.stats = stats or {}
        self._codes, self._offsets, self._consensus = codes, offsets, consensus

    def __len__(self):
        return len(self.scores)

    def domains_of(self, q: int) -> np.ndarray:
        return self.domains[int(self.domain_offsets[q]):int(self.domain_offsets[q + 1])]

    def ops_of(self, d) -> bytes:
        return self.ops[int(d["ops_begin"]):int(d["ops_begin"]) + int(d["ops_len"])].tobytes()

    def path(self, q: int):
        """The core states of entry q's path in order, as (state, k, i) with state in 'MID' (a D keeps the i of
        the residue before it); the specials follow from the domains."""
        for d in self.domains_of(q):
            i, k = int(d["i_from"]) - 1, int(d["k_from"]) - 1
            for op in self.ops_of(d):
                if op == 77:    # M
                    i, k = i + 1, k + 1
                elif op == 73:  # I
                    i += 1
                else:           # D
                    k += 1
                yield chr(op), k, i

    def alignment(self, q: int, d: int) -> str:
        """Domain d of entry q as three lines: the model's consensus residues ('.' opposite an insert), a match
        line ('|' identical, '+' a positive match score, ' ' otherwise) and the sequence ('-' opposite a delete)."""
        if self._codes is None or self._consensus is None:
            raise ValueError("these traces carry no sequences or model to align")
        dom = self.domains_of(q)[d]
        o0 = int(self._offsets[int(dom["seq"])])
        cons, positive = self._consensus
        top, mid, bot = [], [], []
        i, k = int(dom["i_from"]) - 1, int(dom["k_from"]) - 1
        for op in self.ops_of(dom):
            if op == 77:
                i, k = i + 1, k + 1
                r = int(self._codes[o0 + i - 1])
                top.append(AMINO_ACIDS[cons[k]])
                mid.append("|" if r == cons[k] else "+" if positive[r, k] else " ")
                bot.append(AMINO_ACIDS[r])
            elif op == 73:
                i += 1
                top.append(".")
                mid.append(" ")
                bot.append(AMINO_ACIDS[int(self._codes[o0 + i - 1])].lower())
            else:
                k += 1
                top.append(AMINO_ACIDS[cons[k]])
                mid.append(" ")
                bot.append("-")
        return "\n".join("".join(x) for x in (top, mid, bot))


def _cpu_trace(msc, isc, tsc, consts, codes):
    """msv_vit_cpu_trace by its two-call sizing protocol -> (status, score, domains, ops)."""
    L = _native.lib()
    codes = np.ascontiguousarray(codes, np.uint8)
    sc, nd, no = C.c_float(), C.c_uint32(), C.c_uint64()
    args = (msc.ctypes.data, None if isc is None else isc.ctypes.data, tsc.ctypes.data, msc.shape[1],
            *[float(x) for x in consts], codes.ctypes.data if codes.size else None, codes.size)
    st = L.msv_vit_cpu_trace(*args, C.byref(sc), C.byref(nd), C.byref(no), None, None)
    doms = np.zeros(nd.value if st == 0 else 0, _native.DOMAIN_DTYPE)
    ops = np.zeros(no.value if st == 0 else 0, np.uint8)
    if st == 0 and nd.value:
        st = L.msv_vit_cpu_trace(*args, C.byref(sc), C.byref(nd), C.byref(no), doms.ctypes.data, ops.ctypes.data)
    return st, np.float32(sc.value), doms, ops


class _StageEngine:
    """What Viterbi_HMM and Forward_HMM share: one stage profile (msv_vit_* / msv_fwd_*, the same entry points
    under two prefixes) over the log-odds tables of msv_hmm_viterbi_scores, on one GPU."""

    _prefix = ""  # the C symbols' prefix
    _Info = None  # the describe struct

    @classmethod
    def _fn(cls, name: str):
        return getattr(_native.lib(), f"{cls._prefix}_{name}")

    def __init__(self, base_hmm: Profile_HMM, device: int = 0, insert_mode: int = INSERTS_ZERO):
        M = base_hmm.model_length
        self.model_length = M
        self.insert_mode = insert_mode
        self.match_scores = np.zeros((20, M), np.float32)
        self.insert_scores = np.zeros((20, M), np.float32)
        self.transition_scores = np.zeros((M, 7), np.float32)
        b, c, j = C.c_float(), C.c_float(), C.c_float()
        check(_native.lib().msv_hmm_viterbi_scores(
            base_hmm._h, insert_mode, self.match_scores.ctypes.data, self.insert_scores.ctypes.data,
            self.transition_scores.ctypes.data, C.byref(b), C.byref(c), C.byref(j)), "msv_hmm_viterbi_scores")
        self.tr_B_Mk, self.tr_E_C, self.tr_E_J = b.value, c.value, j.value
        p = C.c_void_p()
        check(self._fn("profile_create")(device, *self._tables(), C.byref(p)), f"{self._prefix}_profile_create")
        self._p = p
        self.device = device

    def _tables(self):
        """The model as the create and CPU entry points take it (insert scores NULL for HMMER3's zeros)."""
        return (self.match_scores.ctypes.data, self.insert_scores.ctypes.data if self.insert_mode else None,
                self.transition_scores.ctypes.data, self.model_length, self.tr_B_Mk, self.tr_E_C, self.tr_E_J)

    def parallel_run_on_sequence(self, seq: str) -> float:
        return float(self.score_batch([seq])[0])

    def score_batch(self, seqs: Sequence[str] | None = None, *, codes: np.ndarray | None = None,
                    offsets: np.ndarray | None = None) -> np.ndarray:
        """This stage's scores of every sequence of a host batch (msv_*_score_batch, one launch)."""
        codes, offsets, n = _batch(seqs, codes, offsets)
        out = np.zeros(n, np.float32)
        _check_residues(self._fn("score_batch")(self._p, _ptr(codes), offsets.ctypes.data, n, out.ctypes.data, None),
                        f"{self._prefix}_score_batch")
        return out

    def score_batch_device(self, residues_ptr: int, residues_len: int, offsets_ptr: int, n: int, scores_ptr: int,
                           select_ptr: int | None = None, select_count_ptr: int | None = None,
                           stream: int | None = None) -> None:
        """Device-resident batch (raw device pointers), optionally only the sequences listed at select_ptr
        (uint32; their count in the device uint32 at select_count_ptr, else n); async on `stream`."""
        check(self._fn("score_batch_device")(self._p, residues_ptr, residues_len, offsets_ptr, n, select_ptr,
                                             select_count_ptr, scores_ptr, stream),
              f"{self._prefix}_score_batch_device")

    def reserve_length(self, max_length: int) -> None:
        check(self._fn("profile_reserve_length")(self._p, max_length))

    def bind_stream(self, stream: int | None) -> None:
        """msv_*_profile_bind_stream: launches on this (caller-kept-alive) stream skip the slot event."""
        check(self._fn("profile_bind_stream")(self._p, stream), f"{self._prefix}_profile_bind_stream")

    def check(self, stream: int | None = None) -> None:
        _check_residues(self._fn("profile_check")(self._p, stream), f"{self._prefix}_profile_check")

    def set_variant(self, name: str) -> None:
        check(self._fn("profile_set_variant")(self._p, name.encode()), f"set_variant({name})")

    @classmethod
    def variants(cls) -> list[str]:
        return [cls._fn("variant_name")(i).decode() for i in range(cls._fn("variant_count")())]

    def describe(self) -> dict:
        info = self._Info()
        check(self._fn("profile_describe")(self._p, C.byref(info)))
        return info.as_dict()

    def close(self):
        lib = _loaded_lib()
        if getattr(self, "_p", None) and lib is not None:
            getattr(lib, f"{self._prefix}_profile_destroy")(self._p)
            self._p = None

    def __del__(self):
        self.close()


class Viterbi_HMM(_StageEngine):
    """Viterbi stage for one profile on one GPU: HMMER3's generic local Viterbi over the
    reference's parse (insert emissions, 7 transitions per node: Profile_HMM.cpp:107-120) with the MSV
    path's specials (MSV_HMM.cpp:49-64); msv.h states the recurrence.  Every score comes from the gfx950
    kernel (vit_kernel.hip) except run_on_sequence, which -- like the reference's MSV run_on_sequence --
    is the library's serial CPU DP.  P-values use STATS LOCAL VITERBI (Profile_HMM.cpp:86-87)."""

    _prefix, _Info = "msv_vit", _native.VitInfo

    def __init__(self, base_hmm: Profile_HMM, device: int = 0, insert_mode: int = INSERTS_ZERO):
        super().__init__(base_hmm, device, insert_mode)
        self.viterbi_mu = base_hmm.stats_local_viterbi_mu
        self.viterbi_lambda = base_hmm.stats_local_viterbi_lambda

    def run_on_sequence(self, seq: str) -> float:
        """The serial CPU Viterbi (msv_vit_cpu_score); IndexError on a residue outside the 20."""
        codes = encode(seq[1:] if seq.startswith("#") else seq)
        out = C.c_float()
        check(_native.lib().msv_vit_cpu_score(*self._tables(), _ptr(codes), codes.size, C.byref(out)),
              "msv_vit_cpu_score")
        return out.value

    def _consensus(self):
        return self.match_scores.argmax(axis=0), self.match_scores > 0

    def trace_batch(self, seqs: Sequence[str] | None = None, *, codes: np.ndarray | None = None,
                    offsets: np.ndarray | None = None, select=None, workspace_bytes: int = 0,
                    strict: bool = True) -> Traces:
        """Score and one optimal path of the selected sequences (all when select is None), computed on the GPU
        (msv_vit_trace_batch), per select entry in the caller's order.  workspace_bytes bounds the device memory
        for back-pointers (0: the default of trace_describe()); the call runs in as many chunks as that takes.
        A bad residue raises IndexError as score_batch does, unless strict=False: then the traces are returned
        with `status` set, the bad entries without domains."""
        codes, offsets, n = _batch(seqs, codes, offsets)
        sel = None if select is None else np.ascontiguousarray(select, np.uint32)
        sel_buf = sel if sel is None or sel.size else np.zeros(1, np.uint32)  # (an empty list is not "every one")
        L = _native.lib()
        t = C.c_void_p()
        st = L.msv_vit_trace_batch(self._p, _ptr(codes), offsets.ctypes.data, n,
                                   None if sel is None else sel_buf.ctypes.data,
                                   0 if sel is None else sel.size, workspace_bytes, C.byref(t))
        if not t.value:
            check(st, "msv_vit_trace_batch")
        try:
            if strict:
                _check_residues(st, "msv_vit_trace_batch")
            m = L.msv_vit_traces_count(t)
            scores = np.zeros(m, np.float32)
            dom_off = np.zeros(m + 1, np.uint64)
            doms = np.zeros(L.msv_vit_traces_domains(t), _native.DOMAIN_DTYPE)
            ops = np.zeros(L.msv_vit_traces_ops(t), np.uint8)
            check(L.msv_vit_traces_copy(t, scores.ctypes.data, dom_off.ctypes.data, doms.ctypes.data,
                                        ops.ctypes.data), "msv_vit_traces_copy")
            stats = _native.VitTraceStats()
            check(L.msv_vit_traces_stats(t, C.byref(stats)))
        finally:
            L.msv_vit_traces_free(t)
        return Traces(scores, dom_off, doms, ops, status=_native.STATUS.get(st, str(st)),
                      stats={f: getattr(stats, f) for f, _ in stats._fields_}, codes=codes, offsets=offsets,
                      consensus=self._consensus())

    def trace_on_sequence(self, seq=None, *, codes: np.ndarray | None = None) -> Traces:
        """The serial CPU trace of one sequence (msv_vit_cpu_trace): the same path as trace_batch, bit for bit."""
        if seq is not None:
            codes = encode(seq[1:] if seq.startswith("#") else seq)
        codes = np.ascontiguousarray(codes, np.uint8)
        st, sc, doms, ops = _cpu_trace(self.match_scores, self.insert_scores if self.insert_mode else None,
                                       self.transition_scores, (self.tr_B_Mk, self.tr_E_C, self.tr_E_J), codes)
        _check_residues(st, "msv_vit_cpu_trace")
        return Traces(np.array([sc], np.float32), np.array([0, len(doms)], np.uint64), doms, ops, codes=codes,
                      offsets=np.array([0, codes.size], np.uint64), consensus=self._consensus())

    @staticmethod
    def trace_plans() -> list[tuple[str, int]]:
        """The compiled trace plans as (name, capacity in states), by rising capacity."""
        L = _native.lib()
        return [(L.msv_vit_trace_plan_name(i).decode(), int(L.msv_vit_trace_plan_capacity(i)))
                for i in range(L.msv_vit_trace_plan_count())]

    def trace_describe(self) -> dict:
        info = _native.VitTraceInfo()
        check(_native.lib().msv_vit_trace_describe(self._p, C.byref(info)), "msv_vit_trace_describe")
        return info.as_dict()

    def pvalues(self, scores: np.ndarray, offsets: np.ndarray) -> np.ndarray:
        """P-values of Viterbi scores against STATS LOCAL VITERBI (HMMER3's formula, msv_pvalues)."""
        return _pvalues("msv_pvalues", scores, offsets, self.viterbi_mu, self.viterbi_lambda)


def _sub_batch(codes: np.ndarray, offsets: np.ndarray, idx: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """The CSR batch of the sequences idx of a batch, in that order."""
    lens = (offsets[1:] - offsets[:-1])[idx]
    sub_off = np.zeros(len(idx) + 1, np.uint64)
    np.cumsum(lens, out=sub_off[1:])
    parts = [codes[int(offsets[i]):int(offsets[i + 1])] for i in idx]
    return (np.concatenate(parts) if parts else np.zeros(0, np.uint8)), sub_off


def _filter_pipeline_bias(msv_engine, vit_engine, bias_engine, codes, offsets, n, F1, align, stats, six):
    """filter_pipeline with the bias filter: HMMER3's two MSV-stage tests, Viterbi on the survivors of both (every
    kernel scores a sequence independently of its batch, so the sub-batches give the cascade's own scores)."""
    msc, _, mask, bias = msv_engine.msv_filter(codes=codes, offsets=offsets, F1=F1, bias=bias_engine, stats=stats)
    idx = np.flatnonzero(mask)
    vsc = np.full(n, -np.inf, np.float32)
    vpv = np.full(n, np.nan)
    if idx.size:
        sub_codes, sub_off = _sub_batch(codes, offsets, idx)
        vsc[idx] = vit_engine.score_batch(codes=sub_codes, offsets=sub_off)
        vpv[idx] = bias_engine.pvalues(vsc, bias, offsets, six[2], six[3], kind="gumbel")[idx]
    if align:
        traces = vit_engine.trace_batch(codes=codes, offsets=offsets, select=idx.astype(np.uint32))
        return msc, mask, vsc, vpv, bias, traces
    return msc, mask, vsc, vpv, bias


def filter_pipeline(msv_engine: MSV_HMM, vit_engine: Viterbi_HMM, seqs: Sequence[str] | None = None, *,
                    codes: np.ndarray | None = None, offsets: np.ndarray | None = None, F1: float = 0.02,
                    align: bool = False, bias_engine: "Bias_filter | None" = None, stats=None):
    """HMMER3's MSV -> Viterbi cascade on the GPU (msv_vit_filter_batch): MSV scores of every sequence,
    the survivors P <= F1 (STATS LOCAL MSV), their Viterbi scores (-inf elsewhere) and Viterbi P-values
    (STATS LOCAL VITERBI, NaN elsewhere).  Returns (msv_scores, passed, vit_scores, vit_pvalues); with
    align=True also the Traces of the sequences that passed, in index order (a second call that uploads the
    batch again: Viterbi_HMM.trace_batch with select = the passed indices).  With bias_engine (a Bias_filter) the
    survivors also pass the filtered test (MSV_HMM.msv_filter(bias=)), the Viterbi P-values are the filtered ones
    and the bias [n] is returned after vit_pvalues: (msv_scores, passed, vit_scores, vit_pvalues, bias[, traces]).
    stats (a Calibration, e.g. calibrate()'s, or six floats in msv_hmm_stats' order) replaces the engines' file
    values in every test and P-value; with stats=None nothing changes."""
    codes, offsets, n = _batch(seqs, codes, offsets)
    six = (msv_engine.msv_mu, msv_engine.msv_lambda, vit_engine.viterbi_mu, vit_engine.viterbi_lambda, 0.0, 0.0) \
        if stats is None else _six_stats(stats)
    if bias_engine is not None:
        return _filter_pipeline_bias(msv_engine, vit_engine, bias_engine, codes, offsets, n, F1, align, stats, six)
    msc = np.zeros(n, np.float32)
    passed = np.zeros(n, np.uint8)
    vsc = np.zeros(n, np.float32)
    npass = C.c_uint64(0)
    _check_residues(_native.lib().msv_vit_filter_batch(
        msv_engine._p, vit_engine._p, _ptr(codes), offsets.ctypes.data, n, six[0], six[1],
        F1, msc.ctypes.data, passed.ctypes.data, vsc.ctypes.data, C.byref(npass)), "msv_vit_filter_batch")
    mask = passed.astype(bool)
    vpv = np.full(n, np.nan)
    if mask.any():
        vpv[mask] = _pvalues("msv_pvalues", vsc, offsets, six[2], six[3])[mask]
    if align:
        traces = vit_engine.trace_batch(codes=codes, offsets=offsets, select=np.flatnonzero(mask).astype(np.uint32))
        return msc, mask, vsc, vpv, traces
    return msc, mask, vsc, vpv


class Forward_HMM(_StageEngine):
    """Forward stage for one profile on one GPU (msv.h "Forward stage"): the log, in nats, of the summed
    odds of EVERY alignment -- the score HMMER3's E-values come from.  Same tables and specials as Viterbi_HMM, plus
    the D_k -> E exits.  Every score comes from the gfx950 kernel (fwd_kernel.hip, float32 odds with exact
    power-of-two rescaling) except run_on_sequence, the library's serial float64 CPU Forward, which every test
    compares against.  P-values use STATS LOCAL FORWARD."""

    _prefix, _Info = "msv_fwd", _native.FwdInfo

    def __init__(self, base_hmm: Profile_HMM, device: int = 0, insert_mode: int = INSERTS_ZERO):
        super().__init__(base_hmm, device, insert_mode)
        self.forward_tau = base_hmm.stats_local_forward_theta
        self.forward_lambda = base_hmm.stats_local_forward_lambda

    def run_on_sequence(self, seq: str) -> float:
        """The serial float64 CPU Forward (msv_fwd_cpu_score); IndexError on a residue outside the 20."""
        codes = encode(seq[1:] if seq.startswith("#") else seq)
        out = C.c_double()
        check(_native.lib().msv_fwd_cpu_score(*self._tables(), _ptr(codes), codes.size, C.byref(out)),
              "msv_fwd_cpu_score")
        return out.value

    def cpu_score_batch(self, seqs: Sequence[str] | None = None, *, codes: np.ndarray | None = None,
                        offsets: np.ndarray | None = None) -> np.ndarray:
        """run_on_sequence over a host batch (msv_fwd_cpu_score_batch, a few host threads) -> float64 [n]."""
        codes, offsets, n = _batch(seqs, codes, offsets)
        out = np.zeros(n, np.float64)
        _check_residues(_native.lib().msv_fwd_cpu_score_batch(*self._tables(), _ptr(codes), offsets.ctypes.data, n,
                                                              out.ctypes.data), "msv_fwd_cpu_score_batch")
        return out

    def pvalues(self, scores: np.ndarray, offsets: np.ndarray) -> np.ndarray:
        """P-values of Forward scores against STATS LOCAL FORWARD (msv_fwd_pvalues)."""
        return _pvalues("msv_fwd_pvalues", scores, offsets, self.forward_tau, self.forward_lambda)

    def pvalues_device(self, scores_ptr: int, offsets_ptr: int, n: int, pvalues_ptr: int,
                       stream: int | None = None) -> None:
        """Device P-values (float64 out) for device scores/offsets, async on `stream`."""
        check(_native.lib().msv_fwd_pvalues_device(self.device, scores_ptr, offsets_ptr, n, self.forward_tau,
                                                   self.forward_lambda, pvalues_ptr, stream), "msv_fwd_pvalues_device")


def background_frequencies() -> np.ndarray:
    """The 20 background frequencies every log-odds score of the library is taken against (float32)."""
    return np.ctypeslib.as_array(_native.lib().msv_background_frequencies(), (20,)).copy()


class Bias_filter:
    """HMMER3's bias (composition) filter for one profile on one GPU (msv.h "Bias filter"): the Forward
    score, in nats, of a two-state HMM -- background / the profile's COMPO composition -- over each sequence, which
    replaces null1 in the P-values of the MSV, Viterbi and Forward filters.  Every score comes from the gfx950 kernel
    (bias_filter.hip) except cpu_score, the float64 definition every test compares against.  `profile` is a
    Profile_HMM, or a (compo[20], background[20], model_length) triple of raw arrays."""

    def __init__(self, profile, device: int = 0):
        L = _native.lib()
        if isinstance(profile, Profile_HMM):
            self.compo = np.ascontiguousarray(profile.compo, np.float32)
            self.background = background_frequencies()
            self.model_length = int(profile.model_length)
            self._stats = {"msv": (profile.stats_local_msv_mu, profile.stats_local_msv_lambda),
                           "viterbi": (profile.stats_local_viterbi_mu, profile.stats_local_viterbi_lambda),
                           "forward": (profile.stats_local_forward_theta, profile.stats_local_forward_lambda)}
        else:
            self._stats = {}
            compo, background, model_length = profile
            self.compo = np.ascontiguousarray(compo, np.float32)
            self.background = np.ascontiguousarray(background, np.float32)
            self.model_length = int(model_length)
        if self.compo.shape != (20,) or self.background.shape != (20,):
            raise ValueError("compo and background are 20 values each")
        p = C.c_void_p()
        check(L.msv_bf_profile_create(device, self.compo.ctypes.data, self.background.ctypes.data, self.model_length,
                                      C.byref(p)), "msv_bf_profile_create")
        self._p = p
        self.device = device

    @staticmethod
    def tolerance(lengths, cpu) -> np.ndarray:
        """msv.h's bound on |device - cpu_score| for sequences of these lengths and float64 scores."""
        L = np.asarray(lengths, np.float64)
        k = 5.0 * L + 14.0 * np.ceil(L / 1024.0) + 4.0
        u = 2.0 ** -24
        return k * u / (1.0 - k * u) + u * np.abs(np.asarray(cpu, np.float64))

    def cpu_score(self, seqs: Sequence[str] | None = None, *, codes: np.ndarray | None = None,
                  offsets: np.ndarray | None = None) -> np.ndarray:
        """The float64 definition (msv_bf_cpu_score_batch) over a host batch -> float64 [n]."""
        codes, offsets, n = _batch(seqs, codes, offsets)
        out = np.zeros(n, np.float64)
        _check_residues(_native.lib().msv_bf_cpu_score_batch(
            self.compo.ctypes.data, self.background.ctypes.data, self.model_length, _ptr(codes), offsets.ctypes.data,
            n, out.ctypes.data), "msv_bf_cpu_score_batch")
        return out

    def score_batch(self, seqs: Sequence[str] | None = None, *, codes: np.ndarray | None = None,
                    offsets: np.ndarray | None = None, select: np.ndarray | None = None) -> np.ndarray:
        """The bias of every sequence of a host batch (msv_bf_score_batch, one launch) -> float32 [n].  With
        `select` (indices) only those are scored, as a sub-batch; the others' entries are 0."""
        codes, offsets, n = _batch(seqs, codes, offsets)
        if select is not None:
            idx = np.asarray(select, np.int64)
            out = np.zeros(n, np.float32)
            if idx.size:
                sub_codes, sub_off = _sub_batch(codes, offsets, idx)
                out[idx] = self.score_batch(codes=sub_codes, offsets=sub_off)
            return out
        out = np.zeros(n, np.float32)
        _check_residues(_native.lib().msv_bf_score_batch(self._p, _ptr(codes), offsets.ctypes.data, n,
                                                         out.ctypes.data, None), "msv_bf_score_batch")
        return out

    def score_batch_device(self, residues_ptr: int, residues_len: int, offsets_ptr: int, n: int, bias_ptr: int,
                           select_ptr: int | None = None, select_count_ptr: int | None = None,
                           stream: int | None = None) -> None:
        """Device-resident batch (raw device pointers), optionally only the sequences listed at select_ptr
        (uint32; their count in the device uint32 at select_count_ptr, else n); async on `stream`."""
        check(_native.lib().msv_bf_score_batch_device(self._p, residues_ptr, residues_len, offsets_ptr, n, select_ptr,
                                                      select_count_ptr, bias_ptr, stream),
              "msv_bf_score_batch_device")

    def pvalues(self, scores: np.ndarray, bias: np.ndarray, offsets: np.ndarray, location: float | None = None,
                scale: float | None = None, *, kind: str = "msv") -> np.ndarray:
        """Filtered P-values (msv_bf_pvalues) -> float64 [n].  kind "msv", "viterbi" (Gumbel) or "forward"
        (exponential) takes the stage's STATS LOCAL line of the Profile_HMM this filter was made from; kind
        "gumbel" with (location, scale) = (mu, lambda) or "exponential" with (tau, lambda) takes them as given."""
        kinds = {"gumbel": _native.BF_GUMBEL, "exponential": _native.BF_EXPONENTIAL, "msv": _native.BF_GUMBEL,
                 "viterbi": _native.BF_GUMBEL, "forward": _native.BF_EXPONENTIAL}
        if kind not in kinds:
            raise ValueError("kind is 'msv', 'viterbi', 'forward', 'gumbel' or 'exponential'")
        if location is None or scale is None:
            if kind not in self._stats:
                raise ValueError(f"kind {kind!r} needs location and scale")
            location, scale = self._stats[kind]
        scores = np.ascontiguousarray(scores, np.float32)
        bias = np.ascontiguousarray(bias, np.float32)
        offsets = np.ascontiguousarray(offsets, np.uint64)
        n = len(offsets) - 1
        if scores.shape != (n,) or bias.shape != (n,):
            raise ValueError("scores, bias and offsets disagree")
        out = np.zeros(n, np.float64)
        check(_native.lib().msv_bf_pvalues(scores.ctypes.data, bias.ctypes.data, offsets.ctypes.data, n, location,
                                           scale, kinds[kind], out.ctypes.data), "msv_bf_pvalues")
        return out

    def bind_stream(self, stream: int | None) -> None:
        check(_native.lib().msv_bf_profile_bind_stream(self._p, stream), "msv_bf_profile_bind_stream")

    def check(self, stream: int | None = None) -> None:
        _check_residues(_native.lib().msv_bf_profile_check(self._p, stream), "msv_bf_profile_check")

    def describe(self) -> dict:
        info = _native.BfInfo()
        check(_native.lib().msv_bf_profile_describe(self._p, C.byref(info)))
        return info.as_dict()

    def close(self):
        lib = _loaded_lib()
        if getattr(self, "_p", None) and lib is not None:
            lib.msv_bf_profile_destroy(self._p)
            self._p = None

    def __del__(self):
        self.close()


class Envelopes:
    """What Domain_HMM.decode_batch returns, per select entry q in the caller's order: forward_scores[q],
    backward_scores[q] (nats), the per-residue posteriors begin / end / occ (float32, compacted: entry q's are
    [residue_offsets[q], residue_offsets[q+1]), residue i at index i - 1) and the regions of the envelope rule
    (REGION_DTYPE records seq, i_from, i_to, expected_domains, mass; entry q's are [region_offsets[q],
    region_offsets[q+1])).  `select` are the batch indices of the entries; `status` is the call's status name."""

    def __init__(self, select, forward_scores, backward_scores, residue_offsets, begin, end, occ, region_offsets,
                 regions, status="MSV_OK", stats=None):
        self.select = select
        self.forward_scores, self.backward_scores = forward_scores, backward_scores
        self.residue_offsets, self.region_offsets = residue_offsets, region_offsets
        self.begin, self.end, self.occ = begin, end, occ
        self.regions = regions
        self.status = status
        self.stats = stats or {}

    def __len__(self) -> int:
        return len(self.forward_scores)

    def posteriors(self, q: int):
        """(begin, end, occ) of entry q, float32 [L]."""
        lo, hi = int(self.residue_offsets[q]), int(self.residue_offsets[q + 1])
        return self.begin[lo:hi], self.end[lo:hi], self.occ[lo:hi]

    def regions_of(self, q: int) -> np.ndarray:
        return self.regions[int(self.region_offsets[q]):int(self.region_offsets[q + 1])]


def dom_regions(begin, end, occ, rt1: float = 0.25, rt2: float = 0.10) -> np.ndarray:
    """The envelope rule (msv_dom_regions, THE definition) on three float32 arrays of one sequence -> REGION_DTYPE
    records (seq = 0), by the two-call sizing protocol."""
    b, e, o = (np.ascontiguousarray(x, np.float32) for x in (begin, end, occ))
    if not (b.shape == e.shape == o.shape and b.ndim == 1):
        raise ValueError("begin, end and occ disagree")
    L = _native.lib()
    n = C.c_uint32()
    args = (_ptr(b), _ptr(e), _ptr(o), b.size, rt1, rt2)
    check(L.msv_dom_regions(*args, C.byref(n), None), "msv_dom_regions")
    out = np.zeros(n.value, _native.REGION_DTYPE)
    if n.value:
        check(L.msv_dom_regions(*args, C.byref(n), out.ctypes.data), "msv_dom_regions")
    return out


class Alignments:
    """What Domain_HMM.align_batch returns, per item q in the caller's order (msv.h "Alignment stage"): `items`
    (ITEM_DTYPE records seq, i_from, i_to), envelope_scores[q] = log Z of the envelope (nats), domain_scores[q] =
    HMMER's per-domain score, the envelope score plus (Lc - Le) log(loop) for the flanks, oa_scores[q] = the expected
    number of correctly labelled residues of the optimal-accuracy path and accuracy[q] = oa / Le; the path as the
    Viterbi trace reports one (`domains`, DOMAIN_DTYPE records with the parent's seq and residues relative to the
    parent, entry q's are domains[domain_offsets[q]:domain_offsets[q+1]]; `ops`, one byte 'M' / 'I' / 'D' per core
    state visited) and `op_pp`, one float32 per op: the posterior of the op's cell (0 for 'D').  `status` is the
    call's status name, `stats` what the device did.  Made with null2=True (msv.h "Bias stage") it also has `null2`
    float32 [m, 20], the envelope's null2 odds of each residue, and `domcorrection` float32 [m] (nats), and
    bias_scores gives the corrected bit scores and P-values; else both are None."""

    def __init__(self, items, envelope_scores, domain_scores, oa_scores, domain_offsets, domains, ops, op_pp, *,
                 status="MSV_OK", stats=None, posteriors=None, null2=None, domcorrection=None, parent_lengths=None):
        self.null2, self.domcorrection = null2, domcorrection
        self._parent_lengths = parent_lengths
        self.items = items
        self.envelope_scores, self.domain_scores, self.oa_scores = envelope_scores, domain_scores, oa_scores
        Le = (items["i_to"].astype(np.int64) - items["i_from"].astype(np.int64) + 1).astype(np.float32)
        self.accuracy = (oa_scores / np.maximum(Le, 1)).astype(np.float32)
        self.domain_offsets, self.domains, self.ops, self.op_pp = domain_offsets, domains, ops, op_pp
        self.status = status
        self.stats = stats or {}
        self._posteriors = posteriors

    def __len__(self) -> int:
        return len(self.envelope_scores)

    def domains_of(self, q: int) -> np.ndarray:
        return self.domains[int(self.domain_offsets[q]):int(self.domain_offsets[q + 1])]

    def ops_of(self, d) -> bytes:
        return self.ops[int(d["ops_begin"]):int(d["ops_begin"]) + int(d["ops_len"])].tobytes()

    def pp_of(self, d) -> np.ndarray:
        return self.op_pp[int(d["ops_begin"]):int(d["ops_begin"]) + int(d["ops_len"])]

    def pp_line(self, d) -> str:
        """HMMER's PP line of a domain, one character per op: '*' if p + 0.05 >= 1, else the digit int(10 p + 0.5);
        '.' opposite a delete, which emits no residue."""
        out = []
        for op, p in zip(self.ops_of(d), self.pp_of(d)):
            out.append("." if op == 68 else "*" if float(p) + 0.05 >= 1.0 else str(int(10.0 * float(p) + 0.5)))
        return "".join(out)

    def posteriors(self, q: int):
        """(ppM, ppI, ppN, ppJ, ppC) of item q as the device computed them (keep_posteriors=True): ppM, ppI float32
        [Le, LENG + 1] (row i - 1, column k), the others float32 [Le]."""
        if self._posteriors is None:
            raise ValueError("these alignments were made without keep_posteriors")
        return self._posteriors[q]

    def bias_scores(self, tau: float, lam: float, fwd_scores=None) -> dict:
        """The bias-corrected scores (msv_aln_bias_scores; tau, lam = STATS LOCAL FORWARD): dombias, domain_bits
        (float32 [m]) and domain_pvalues (float64 [m]).  With fwd_scores -- the Forward scores of the batch's
        sequences, indexed as items["seq"] is -- also seq_bias, seq_bits, seq_pvalues over those sequences, each
        sequence's bias taken from the summed corrections of its items."""
        if self.domcorrection is None:
            raise ValueError("these alignments were made without null2")
        m = len(self)
        Lc = np.ascontiguousarray(self._parent_lengths[self.items["seq"].astype(np.int64)] if m else [], np.uint64)
        Le = np.ascontiguousarray(self.items["i_to"].astype(np.int64) - self.items["i_from"].astype(np.int64) + 1,
                                  np.uint64)
        env = np.ascontiguousarray(self.envelope_scores, np.float32)
        dc = np.ascontiguousarray(self.domcorrection, np.float32)
        parent = np.ascontiguousarray(self.items["seq"], np.uint32)
        out = {"dombias": np.zeros(m, np.float32), "domain_bits": np.zeros(m, np.float32),
               "domain_pvalues": np.zeros(m, np.float64)}
        n_seq, fwd, lens = 0, None, None
        if fwd_scores is not None:
            fwd = np.ascontiguousarray(fwd_scores, np.float32)
            n_seq = fwd.size
            if n_seq != self._parent_lengths.size:
                raise ValueError("fwd_scores must have one score per sequence of the batch")
            lens = np.ascontiguousarray(self._parent_lengths, np.uint64)
            out.update(seq_bias=np.zeros(n_seq, np.float32), seq_bits=np.zeros(n_seq, np.float32),
                       seq_pvalues=np.zeros(n_seq, np.float64))
        check(_native.lib().msv_aln_bias_scores(
            _ptr(env), _ptr(Le), _ptr(Lc), _ptr(dc), m, _ptr(parent), None if fwd is None else _ptr(fwd),
            None if lens is None else _ptr(lens), n_seq, tau, lam, _ptr(out["dombias"]), _ptr(out["domain_bits"]),
            _ptr(out["domain_pvalues"]), *[_ptr(out[k]) if k in out else None
                                           for k in ("seq_bias", "seq_bits", "seq_pvalues")]),
            "msv_aln_bias_scores")
        return out


def aln_oa(ppM, ppI, ppN, ppJ, ppC, transition_scores, consts, Lc: int | None = None):
    """THE definition of the optimal-accuracy alignment (msv_aln_oa) on float32 posteriors of one envelope: ppM, ppI
    [Le, LENG + 1], ppN, ppJ, ppC [Le]; consts = (tr_B_Mk, tr_E_C, tr_E_J); Lc the configured length (default Le).
    Returns (oa score, domains, ops, op_pp) by the two-call sizing protocol, i relative to the envelope."""
    pm, pi, pn, pj, pc = (np.ascontiguousarray(x, np.float32) for x in (ppM, ppI, ppN, ppJ, ppC))
    tsc = np.ascontiguousarray(transition_scores, np.float32)
    Le, M = pn.size, tsc.shape[0]
    if not (pm.shape == pi.shape == (Le, M) and pj.shape == pc.shape == (Le,) and tsc.shape == (M, 7)):
        raise ValueError("posterior arrays and transition scores disagree")
    L = _native.lib()
    sc, nd, no = C.c_float(), C.c_uint32(), C.c_uint64()
    args = (_ptr(pm), _ptr(pi), _ptr(pn), _ptr(pj), _ptr(pc), tsc.ctypes.data, M, *[float(x) for x in consts], Le,
            Le if Lc is None else Lc)
    check(L.msv_aln_oa(*args, C.byref(sc), C.byref(nd), C.byref(no), None, None, None), "msv_aln_oa")
    doms = np.zeros(nd.value, _native.DOMAIN_DTYPE)
    ops, pp = np.zeros(no.value, np.uint8), np.zeros(no.value, np.float32)
    if nd.value:
        check(L.msv_aln_oa(*args, C.byref(sc), C.byref(nd), C.byref(no), doms.ctypes.data, ops.ctypes.data,
                           pp.ctypes.data), "msv_aln_oa")
    return np.float32(sc.value), doms, ops, pp


def _items_of(items, envelopes, what: str) -> np.ndarray:
    """The ITEM_DTYPE records of (seq, i_from, i_to) triples or records, or of every region of an Envelopes."""
    if envelopes is not None:
        if items is not None:
            raise ValueError("give items or envelopes, not both")
        reg = envelopes.regions
        it = np.zeros(len(reg), _native.ITEM_DTYPE)
        it["seq"], it["i_from"], it["i_to"] = reg["seq"], reg["i_from"], reg["i_to"]
    elif items is None:
        raise ValueError(f"{what} needs items or envelopes")
    else:
        src = np.asarray(items)
        if src.dtype.names:
            it = np.zeros(len(src), _native.ITEM_DTYPE)
            for f in ("seq", "i_from", "i_to"):
                it[f] = src[f]
        else:
            src = src.reshape(-1, 3)
            if src.size and (src.min() < 0 or src.max() >= 2 ** 32):
                raise ValueError("an item outside 32 bits")
            it = np.zeros(len(src), _native.ITEM_DTYPE)
            it["seq"], it["i_from"], it["i_to"] = src[:, 0], src[:, 1], src[:, 2]
    return np.ascontiguousarray(it)


def dom_is_multidomain(begin, end, i_from: int, i_to: int, rt3: float = 0.20) -> bool:
    """HMMER3's is_multidomain_region (msv_dom_is_multidomain, THE definition) on the float32 begin / end arrays of
    one sequence (residue i at index i - 1) for the region i_from .. i_to."""
    b, e = (np.ascontiguousarray(x, np.float32) for x in (begin, end))
    if not (b.shape == e.shape and b.ndim == 1):
        raise ValueError("begin and end disagree")
    out = C.c_int()
    check(_native.lib().msv_dom_is_multidomain(_ptr(b), _ptr(e), b.size, int(i_from), int(i_to), rt3, C.byref(out)),
          "msv_dom_is_multidomain")
    return bool(out.value)


def _cluster_options(min_overlap=0.8, max_diagdiff=4, min_posterior=0.25, min_endpointp=0.02):
    """msv_spl_cluster_options: every fraction as the integer ratio the library tests with."""
    from fractions import Fraction
    o = _native.SplClusterOptions()
    for name, x in (("min_overlap", min_overlap), ("min_posterior", min_posterior), ("min_endpointp", min_endpointp)):
        f = Fraction(x).limit_denominator(10000)
        if not 0 <= f <= 1:
            raise ValueError(f"{name} outside [0, 1]")
        setattr(o, name + "_num", f.numerator)
        setattr(o, name + "_den", f.denominator)
    if int(max_diagdiff) < 1:
        raise ValueError("max_diagdiff must be at least 1")
    o.max_diagdiff = int(max_diagdiff)
    return o


def spl_cluster(segments, n_samples: int, **options) -> np.ndarray:
    """HMMER3's single-linkage clustering of sampled domains (msv_spl_cluster, THE definition) on the SEGMENT_DTYPE
    records of one item's samples -> SPLIT_ENVELOPE_DTYPE records sorted by i_from.  Options: min_overlap=0.8,
    max_diagdiff=4, min_posterior=0.25, min_endpointp=0.02."""
    seg = np.ascontiguousarray(segments, _native.SEGMENT_DTYPE)
    o = _cluster_options(**options)
    L = _native.lib()
    n = C.c_uint32()
    check(L.msv_spl_cluster(_ptr(seg), len(seg), int(n_samples), C.byref(o), C.byref(n), None), "msv_spl_cluster")
    out = np.zeros(n.value, _native.SPLIT_ENVELOPE_DTYPE)
    if n.value:
        check(L.msv_spl_cluster(_ptr(seg), len(seg), int(n_samples), C.byref(o), C.byref(n), out.ctypes.data),
              "msv_spl_cluster")
    return out


def spl_sample(fM, fI, fD, records, transition_scores, consts, *, Lc: int, seq: int, i_from: int, i_to: int,
               sample: int, seed: int = 42):
    """THE definition of one stochastic traceback sample (msv_spl_sample) on the recorded planes of one envelope: fM,
    fI, fD float32 [Le, LENG + 1], records uint32 [Le + 1, 6]; consts = (tr_B_Mk, tr_E_C, tr_E_J).  Returns
    (segments with residues relative to the parent, domains and ops relative to the envelope, truncated)."""
    pm, pi, pd = (np.ascontiguousarray(x, np.float32) for x in (fM, fI, fD))
    rec = np.ascontiguousarray(records, np.uint32)
    tsc = np.ascontiguousarray(transition_scores, np.float32)
    Le, M = int(i_to) - int(i_from) + 1, tsc.shape[0]
    if not (pm.shape == pi.shape == pd.shape == (Le, M) and rec.shape == (Le + 1, 6) and tsc.shape == (M, 7)):
        raise ValueError("planes, records and transition scores disagree")
    L = _native.lib()
    ns, no, tr = C.c_uint32(), C.c_uint64(), C.c_int()
    args = (_ptr(pm), _ptr(pi), _ptr(pd), _ptr(rec), tsc.ctypes.data, M, *[float(x) for x in consts], int(Lc),
            int(seed), int(seq), int(i_from), int(i_to), int(sample))
    check(L.msv_spl_sample(*args, C.byref(ns), C.byref(no), C.byref(tr), None, None, None), "msv_spl_sample")
    segs = np.zeros(ns.value, _native.SEGMENT_DTYPE)
    doms = np.zeros(ns.value, _native.DOMAIN_DTYPE)
    ops = np.zeros(no.value, np.uint8)
    if ns.value:
        check(L.msv_spl_sample(*args, C.byref(ns), C.byref(no), C.byref(tr), segs.ctypes.data, doms.ctypes.data,
                               ops.ctypes.data), "msv_spl_sample")
    return segs, doms, ops, bool(tr.value)


class Ensembles:
    """What Domain_HMM.sample_batch returns, per item q in the caller's order (msv.h "Split stage"): `items`
    (ITEM_DTYPE), envelope_scores[q] (nats), and the sampled domains as SEGMENT_DTYPE records (i_from, i_to relative
    to the parent, k_from, k_to): sample j of item q owns segments[sample_offsets[q n_samples + j] :
    sample_offsets[q n_samples + j + 1]].  `stats` says what the device did (truncated: samples that met a zero
    total weight).  Made with keep_matrix=True, matrix(q) gives the recorded planes."""

    def __init__(self, items, envelope_scores, sample_offsets, segments, n_samples, seed, *, status="MSV_OK",
                 stats=None, matrices=None):
        self.items, self.envelope_scores = items, envelope_scores
        self.sample_offsets, self.segments = sample_offsets, segments
        self.n_samples, self.seed = n_samples, seed
        self.status = status
        self.stats = stats or {}
        self._matrices = matrices

    def __len__(self) -> int:
        return len(self.envelope_scores)

    def segments_of(self, q: int, sample: int | None = None) -> np.ndarray:
        """The segments of every sample of item q, or of one sample."""
        lo = q * self.n_samples if sample is None else q * self.n_samples + sample
        hi = (q + 1) * self.n_samples if sample is None else lo + 1
        return self.segments[int(self.sample_offsets[lo]):int(self.sample_offsets[hi])]

    def matrix(self, q: int):
        """(fM, fI, fD, records) of item q as the device recorded them (keep_matrix=True): the planes float32
        [Le, LENG + 1] in the scale of each row's exponent, records uint32 [Le + 1, 6]."""
        if self._matrices is None:
            raise ValueError("these ensembles were made without keep_matrix")
        return self._matrices[q]

    def cluster(self, q: int | None = None, **options):
        """msv_spl_cluster on item q's segments -> SPLIT_ENVELOPE_DTYPE records; q None: a list, one per item."""
        if q is None:
            return [self.cluster(i, **options) for i in range(len(self))]
        return spl_cluster(self.segments_of(q), self.n_samples, **options)


def _domain_scores(envelope_scores, Le, Lc) -> np.ndarray:
    """envelope score + (Lc - Le) log(loop of Lc): HMMER's per-domain score, float32 adds on float32 values."""
    loops = np.array([sequence_transitions(int(x))[0] for x in Lc], np.float32)
    return (envelope_scores + (np.asarray(Lc, np.float32) - np.asarray(Le, np.float32)) * loops).astype(np.float32)


class Domain_HMM(_StageEngine):
    """Domain stage for one profile on one GPU (msv.h "Domain stage"): Backward, the per-residue domain
    posteriors from Forward x Backward on the special states, and HMMER3's envelope rule on them.  Tables and
    specials are Forward_HMM's.  decode_batch runs on the gfx950 kernels (dom_kernel.hip: the recording Forward
    launch, the Backward launch, the region launches); decode_on_sequence is the library's serial float64 CPU twin,
    which every test compares against.  score_batch returns the recording kernel's Forward score."""

    _prefix, _Info = "msv_dom", _native.DomInfo

    def decode_on_sequence(self, seq=None, *, codes: np.ndarray | None = None):
        """The float64 CPU decode (msv_dom_cpu_decode) -> (forward score, backward score, begin, end, occ), the
        arrays float64 [L]; IndexError on a residue outside the 20."""
        if seq is not None:
            codes = encode(seq[1:] if seq.startswith("#") else seq)
        codes = np.ascontiguousarray(codes, np.uint8)
        f, b = C.c_double(), C.c_double()
        begin, end, occ = (np.zeros(codes.size, np.float64) for _ in range(3))
        _check_residues(_native.lib().msv_dom_cpu_decode(*self._tables(), _ptr(codes), codes.size, C.byref(f),
                                                         C.byref(b), _ptr(begin), _ptr(end), _ptr(occ)),
                        "msv_dom_cpu_decode")
        return f.value, b.value, begin, end, occ

    @staticmethod
    def workspace_bytes(residues_len: int, n: int) -> int:
        """The workspace decode_batch_device needs for a batch of n sequences and residues_len residues."""
        return 24 * (residues_len + n)

    def decode_batch_device(self, residues_ptr: int, residues_len: int, offsets_ptr: int, n: int, fwd_scores_ptr: int,
                            bck_scores_ptr: int, begin_ptr: int, end_ptr: int, occ_ptr: int, workspace_ptr: int,
                            workspace_bytes: int, select_ptr: int | None = None, select_count_ptr: int | None = None,
                            stream: int | None = None) -> None:
        """msv_dom_decode_batch_device on raw device pointers: the recording launch and the Backward launch, async on
        `stream`; scores at the sequence's index, posteriors (float32) at the residue's CSR index."""
        check(_native.lib().msv_dom_decode_batch_device(
            self._p, residues_ptr, residues_len, offsets_ptr, n, select_ptr, select_count_ptr, fwd_scores_ptr,
            bck_scores_ptr, begin_ptr, end_ptr, occ_ptr, workspace_ptr, workspace_bytes, stream),
            "msv_dom_decode_batch_device")

    def decode_batch(self, seqs: Sequence[str] | None = None, *, codes: np.ndarray | None = None,
                     offsets: np.ndarray | None = None, select=None, rt1: float = 0.25, rt2: float = 0.10,
                     workspace_bytes: int = 0, strict: bool = True) -> Envelopes:
        """Scores, posteriors and regions of the selected sequences (all when select is None), computed on the GPU
        (msv_dom_decode_batch), per select entry in the caller's order.  workspace_bytes bounds the device memory
        for the Forward records (0: 1 GiB); the call runs in as many chunks as that takes.  A bad residue raises
        IndexError as score_batch does, unless strict=False: then the result is returned with `status` set."""
        codes, offsets, n = _batch(seqs, codes, offsets)
        sel = None if select is None else np.ascontiguousarray(select, np.uint32)
        sel_buf = sel if sel is None or sel.size else np.zeros(1, np.uint32)  # (an empty list is not "every one")
        L = _native.lib()
        r = C.c_void_p()
        st = L.msv_dom_decode_batch(self._p, _ptr(codes), offsets.ctypes.data, n,
                                    None if sel is None else sel_buf.ctypes.data, 0 if sel is None else sel.size,
                                    rt1, rt2, workspace_bytes, C.byref(r))
        if not r.value:
            check(st, "msv_dom_decode_batch")
        try:
            if strict:
                _check_residues(st, "msv_dom_decode_batch")
            m = L.msv_dom_result_count(r)
            fwd, bck = np.zeros(m, np.float32), np.zeros(m, np.float32)
            res_off, reg_off = np.zeros(m + 1, np.uint64), np.zeros(m + 1, np.uint64)
            begin, end, occ = (np.zeros(L.msv_dom_result_residues(r), np.float32) for _ in range(3))
            regions = np.zeros(L.msv_dom_result_regions(r), _native.REGION_DTYPE)
            check(L.msv_dom_result_copy(r, fwd.ctypes.data, bck.ctypes.data, res_off.ctypes.data, _ptr(begin),
                                        _ptr(end), _ptr(occ), reg_off.ctypes.data, _ptr(regions)),
                  "msv_dom_result_copy")
            stats = _native.DomStats()
            check(L.msv_dom_result_stats(r, C.byref(stats)))
        finally:
            L.msv_dom_result_free(r)
        return Envelopes(np.arange(n, dtype=np.uint32) if sel is None else sel, fwd, bck, res_off, begin, end, occ,
                         reg_off, regions, status=_native.STATUS.get(st, str(st)),
                         stats={f: getattr(stats, f) for f, _ in stats._fields_ if f != "reserved"})

    def align_describe(self) -> dict:
        """msv_aln_describe: the alignment stage's variant, grids and, per kernel, scratch and LDS bytes."""
        info = _native.AlnInfo()
        check(_native.lib().msv_aln_describe(self._p, C.byref(info)), "msv_aln_describe")
        return info.as_dict()

    def align_on_sequence(self, seq=None, *, codes: np.ndarray | None = None, Lc: int | None = None):
        """The CPU twin of the alignment stage for one envelope given as a sequence of its own (msv_aln_cpu_align):
        the float64 decode rounded to float32, then the definition.  Lc is the configured length (default: the
        envelope's).  Returns (envelope score float64, oa score float32, domains, ops, op_pp)."""
        if seq is not None:
            codes = encode(seq[1:] if seq.startswith("#") else seq)
        codes = np.ascontiguousarray(codes, np.uint8)
        L = _native.lib()
        sc, oa, nd, no = C.c_double(), C.c_float(), C.c_uint32(), C.c_uint64()
        args = (*self._tables(), _ptr(codes), codes.size, codes.size if Lc is None else Lc)
        _check_residues(L.msv_aln_cpu_align(*args, C.byref(sc), C.byref(oa), C.byref(nd), C.byref(no), None, None,
                                            None), "msv_aln_cpu_align")
        doms = np.zeros(nd.value, _native.DOMAIN_DTYPE)
        ops, pp = np.zeros(no.value, np.uint8), np.zeros(no.value, np.float32)
        if nd.value:
            check(L.msv_aln_cpu_align(*args, C.byref(sc), C.byref(oa), C.byref(nd), C.byref(no), doms.ctypes.data,
                                      ops.ctypes.data, pp.ctypes.data), "msv_aln_cpu_align")
        return sc.value, np.float32(oa.value), doms, ops, pp

    def posteriors_on_sequence(self, seq=None, *, codes: np.ndarray | None = None, Lc: int | None = None):
        """The float64 CPU decode of one envelope (msv_aln_cpu_decode) -> (score, ppM, ppI, ppN, ppJ, ppC), ppM and
        ppI float64 [Le, LENG + 1]."""
        if seq is not None:
            codes = encode(seq[1:] if seq.startswith("#") else seq)
        codes = np.ascontiguousarray(codes, np.uint8)
        Le, M = codes.size, self.model_length
        sc = C.c_double()
        pm, pi = np.zeros((Le, M), np.float64), np.zeros((Le, M), np.float64)
        pn, pj, pc = (np.zeros(Le, np.float64) for _ in range(3))
        _check_residues(_native.lib().msv_aln_cpu_decode(*self._tables(), _ptr(codes), Le, Le if Lc is None else Lc,
                                                         C.byref(sc), _ptr(pm), _ptr(pi), _ptr(pn), _ptr(pj),
                                                         _ptr(pc)), "msv_aln_cpu_decode")
        return sc.value, pm, pi, pn, pj, pc

    def split_describe(self) -> dict:
        """msv_spl_describe: the split stage's variant, grid and, per kernel, scratch and LDS bytes."""
        info = _native.SplInfo()
        check(_native.lib().msv_spl_describe(self._p, C.byref(info)), "msv_spl_describe")
        return info.as_dict()

    def forward_on_envelope(self, seq=None, *, codes: np.ndarray | None = None, Lc: int | None = None):
        """The float64 twin of the split stage's recording launch (msv_spl_cpu_forward) -> (score, fM, fI, fD
        float64 [Le, LENG + 1], specials float64 [Le + 1, 5] = N, J, C, B, E, exponents int32 [Le + 1])."""
        if seq is not None:
            codes = encode(seq[1:] if seq.startswith("#") else seq)
        codes = np.ascontiguousarray(codes, np.uint8)
        Le, M = codes.size, self.model_length
        sc = C.c_double()
        fm, fi, fd = (np.zeros((Le, M), np.float64) for _ in range(3))
        sp, ex = np.zeros((Le + 1, 5), np.float64), np.zeros(Le + 1, np.int32)
        _check_residues(_native.lib().msv_spl_cpu_forward(*self._tables(), _ptr(codes), Le, Le if Lc is None else Lc,
                                                          C.byref(sc), _ptr(fm), _ptr(fi), _ptr(fd), _ptr(sp),
                                                          _ptr(ex)), "msv_spl_cpu_forward")
        return sc.value, fm, fi, fd, sp, ex

    def sample_batch(self, seqs: Sequence[str] | None = None, items=None, *, codes: np.ndarray | None = None,
                     offsets: np.ndarray | None = None, envelopes: "Envelopes | None" = None, n_samples: int = 200,
                     seed: int = 42, workspace_bytes: int = 0, keep_matrix: bool = False, strict: bool = True,
                     stream: int | None = None) -> Ensembles:
        """Stochastic traceback ensembles of envelopes, on the GPU (msv_spl_sample_batch): per item a recording
        Forward launch that keeps fM, fI and fD, then n_samples alignments sampled from the posterior, of which the
        domains' end points are returned.  Items, envelopes=, workspace_bytes and strict as align_batch.  A sample's
        random numbers are keyed by (seed, seq, i_from, i_to, sample), so an item's samples depend on nothing else."""
        codes, offsets, n = _batch(seqs, codes, offsets)
        it = _items_of(items, envelopes, "sample_batch")
        L = _native.lib()
        r = C.c_void_p()
        opts = _native.SplOptions(workspace_bytes, seed, n_samples, 1 if keep_matrix else 0, stream)
        st = L.msv_spl_sample_batch(self._p, _ptr(codes), offsets.ctypes.data, n, _ptr(it), len(it), C.byref(opts),
                                    C.byref(r))
        if not r.value:
            check(st, "msv_spl_sample_batch")
        try:
            if st not in (_native.MSV_OK, _native.MSV_ERR_BAD_RESIDUE):
                check(st, "msv_spl_sample_batch")
            if strict:
                _check_residues(st, "msv_spl_sample_batch")
            m = L.msv_spl_result_count(r)
            stats = _native.SplStats()
            check(L.msv_spl_result_stats(r, C.byref(stats)))
            ns = stats.n_samples
            env = np.zeros(m, np.float32)
            soff = np.zeros(m * ns + 1, np.uint64)
            segs = np.zeros(L.msv_spl_result_segments(r), _native.SEGMENT_DTYPE)
            check(L.msv_spl_result_copy(r, _ptr(env), soff.ctypes.data, _ptr(segs)), "msv_spl_result_copy")
            mats = None
            if keep_matrix:
                mats = []
                for q in range(m):
                    Le = int(it["i_to"][q]) - int(it["i_from"][q]) + 1
                    fm, fi, fd = (np.zeros((Le, self.model_length), np.float32) for _ in range(3))
                    rec = np.zeros((Le + 1, 6), np.uint32)
                    check(L.msv_spl_result_matrix(r, q, _ptr(fm), _ptr(fi), _ptr(fd), _ptr(rec)),
                          "msv_spl_result_matrix")
                    mats.append((fm, fi, fd, rec))
            stats = {f: getattr(stats, f) for f, _ in stats._fields_ if f != "struct_size"}
        finally:
            L.msv_spl_result_free(r)
        return Ensembles(it, env, soff, segs, ns, stats["seed"], status=_native.STATUS.get(st, str(st)), stats=stats,
                         matrices=mats)

    def split_regions(self, envelopes: "Envelopes", seqs: Sequence[str] | None = None, *,
                      codes: np.ndarray | None = None, offsets: np.ndarray | None = None, rt3: float = 0.20,
                      n_samples: int = 200, seed: int = 42, workspace_bytes: int = 0, **cluster_options) -> dict:
        """HMMER3's treatment of multi-domain regions (msv.h "Split stage"): every region of `envelopes` is tested
        with msv_dom_is_multidomain(rt3) on the entry's begin / end; the multi-domain ones are sampled on the GPU
        (sample_batch) and clustered (msv_spl_cluster), and each is replaced by its clusters' envelopes (none if no
        cluster passes).  Returns {"items": ITEM_DTYPE records for align_batch(items=), in region order; "region":
        the index into envelopes.regions each item came from; "prob": float32, 1 for an unsplit region, else the
        cluster's count / n_samples; "k_from", "k_to": the cluster's node range (0 for an unsplit region);
        "multidomain": bool per region; "ensembles": the Ensembles of the multi-domain regions}."""
        codes, offsets, n = _batch(seqs, codes, offsets)
        reg = envelopes.regions
        multi = np.zeros(len(reg), bool)
        at = 0
        for q in range(len(envelopes)):
            b, e, _ = envelopes.posteriors(q)
            for g in envelopes.regions_of(q):
                multi[at] = dom_is_multidomain(b, e, int(g["i_from"]), int(g["i_to"]), rt3)
                at += 1
        idx = np.flatnonzero(multi)
        sub = np.zeros(len(idx), _native.ITEM_DTYPE)
        sub["seq"], sub["i_from"], sub["i_to"] = reg["seq"][idx], reg["i_from"][idx], reg["i_to"][idx]
        ens = self.sample_batch(codes=codes, offsets=offsets, items=sub, n_samples=n_samples, seed=seed,
                                workspace_bytes=workspace_bytes)
        rows = []
        where = {int(g): j for j, g in enumerate(idx)}
        for g in range(len(reg)):
            if not multi[g]:
                rows.append((int(reg["seq"][g]), int(reg["i_from"][g]), int(reg["i_to"][g]), g, 1.0, 0, 0))
                continue
            for c in ens.cluster(where[g], **cluster_options):
                rows.append((int(reg["seq"][g]), int(c["i_from"]), int(c["i_to"]), g, float(c["prob"]),
                             int(c["k_from"]), int(c["k_to"])))
        it = np.zeros(len(rows), _native.ITEM_DTYPE)
        out = {"items": it, "region": np.zeros(len(rows), np.int64), "prob": np.zeros(len(rows), np.float32),
               "k_from": np.zeros(len(rows), np.uint32), "k_to": np.zeros(len(rows), np.uint32),
               "multidomain": multi, "ensembles": ens}
        for j, (s, a, b, g, pr, kf, kt) in enumerate(rows):
            it[j] = (s, a, b)
            out["region"][j], out["prob"][j], out["k_from"][j], out["k_to"][j] = g, pr, kf, kt
        return out

    def align_batch(self, seqs: Sequence[str] | None = None, items=None, *, codes: np.ndarray | None = None,
                    offsets: np.ndarray | None = None, envelopes: "Envelopes | None" = None,
                    workspace_bytes: int = 0, keep_posteriors: bool = False, strict: bool = True,
                    null2: bool = False) -> Alignments:
        """Posterior decoding and the optimal-accuracy alignment of envelopes, on the GPU (msv_aln_align_batch_opts).
        `items` are (seq, i_from, i_to) triples (1-based, inclusive) or ITEM_DTYPE records; envelopes= takes an
        Envelopes and aligns every region of it.  Each item is decoded as a sequence of its own whose loop / move are
        those of the parent's length.  workspace_bytes bounds the device workspace (0: 1 GiB); keep_posteriors keeps
        the device's posteriors on the host (8 Le (LENG + 1) bytes an item).  A bad residue inside an item raises
        IndexError unless strict=False: then that item has no domains and `status` says so.  null2=True also runs the
        bias stage (msv.h "Bias stage"): the result carries `null2` and `domcorrection`, and bias_scores works."""
        codes, offsets, n = _batch(seqs, codes, offsets)
        it = _items_of(items, envelopes, "align_batch")
        L = _native.lib()
        r = C.c_void_p()
        opts = _native.AlnOptions(workspace_bytes, 1 if keep_posteriors else 0, 1 if null2 else 0)
        st = L.msv_aln_align_batch_opts(self._p, _ptr(codes), offsets.ctypes.data, n, _ptr(it), len(it), C.byref(opts),
                                        C.byref(r))
        if not r.value:
            check(st, "msv_aln_align_batch_opts")
        try:
            if st not in (_native.MSV_OK, _native.MSV_ERR_BAD_RESIDUE):
                check(st, "msv_aln_align_batch_opts")
            if strict:
                _check_residues(st, "msv_aln_align_batch_opts")
            m = L.msv_aln_result_count(r)
            env, oa = np.zeros(m, np.float32), np.zeros(m, np.float32)
            dom_off = np.zeros(m + 1, np.uint64)
            doms = np.zeros(L.msv_aln_result_domains(r), _native.DOMAIN_DTYPE)
            ops = np.zeros(L.msv_aln_result_ops(r), np.uint8)
            pp = np.zeros(len(ops), np.float32)
            check(L.msv_aln_result_copy(r, env.ctypes.data, oa.ctypes.data, dom_off.ctypes.data, _ptr(doms), _ptr(ops),
                                        _ptr(pp)), "msv_aln_result_copy")
            Le = it["i_to"].astype(np.int64) - it["i_from"].astype(np.int64) + 1
            post = None
            if keep_posteriors:
                post = []
                for q in range(m):
                    pm, pi = (np.zeros((int(Le[q]), self.model_length), np.float32) for _ in range(2))
                    pn, pj, pc = (np.zeros(int(Le[q]), np.float32) for _ in range(3))
                    check(L.msv_aln_result_posteriors(r, q, _ptr(pm), _ptr(pi), _ptr(pn), _ptr(pj), _ptr(pc)),
                          "msv_aln_result_posteriors")
                    post.append((pm, pi, pn, pj, pc))
            stats = _native.AlnStats()
            check(L.msv_aln_result_stats(r, C.byref(stats)))
            stats = {f: getattr(stats, f) for f, _ in stats._fields_}
            n2 = dc = None
            if null2:
                n2, dc = np.zeros((m, 20), np.float32), np.zeros(m, np.float32)
                check(L.msv_aln_result_null2(r, _ptr(n2), _ptr(dc)), "msv_aln_result_null2")
                ns = _native.AlnNull2Stats()
                check(L.msv_aln_result_null2_stats(r, C.byref(ns)), "msv_aln_result_null2_stats")
                stats.update(null2_ms=ns.null2_ms, null2_partial_ms=ns.partial_ms, null2_slab_bytes=ns.slab_bytes,
                             null2_row_block=ns.row_block)
        finally:
            L.msv_aln_result_free(r)
        lengths = np.diff(offsets.astype(np.int64))
        Lc = lengths[it["seq"].astype(np.int64)] if m else np.zeros(0, np.int64)
        return Alignments(it, env, _domain_scores(env, Le, Lc), oa, dom_off, doms, ops, pp,
                          status=_native.STATUS.get(st, str(st)), stats=stats, posteriors=post, null2=n2,
                          domcorrection=dc, parent_lengths=lengths)


class Calibration:
    """What calibrate() returns (msv.h "Calibration"): `stats`, float32[6] in msv_hmm_stats' order (MSV
    mu, lambda, Viterbi mu, lambda, Forward tau, lambda) -- the slots of an engine that was not given hold the file's
    values; `lambda_`, the profile's lambda in float64; `report`, the float64 values, the fitted Gumbel, the Newton
    iterations and the chunk counts; `from_file`, the file's own six for comparison; `scores`, per set that ran the
    sample's raw scores when they were asked for.  Pass it as `stats=` to filter_pipeline / search_pipeline."""

    def __init__(self, stats, lambda_, report, from_file, scores=None):
        self.stats = np.asarray(stats, np.float32)
        self.lambda_ = float(lambda_)
        self.report = report
        self.from_file = np.asarray(from_file, np.float32)
        self.scores = scores or {}

    def __repr__(self):
        return f"Calibration(stats={self.stats.tolist()}, from_file={self.from_file.tolist()})"


def _six_stats(stats) -> tuple:
    """A Calibration or six numbers as six Python floats holding float32 values, msv_hmm_stats' order."""
    six = np.asarray(stats.stats if isinstance(stats, Calibration) else stats, np.float32)
    if six.shape != (6,):
        raise ValueError("stats is a Calibration or six floats")
    return tuple(float(x) for x in six)


def _file_stats(profile: Profile_HMM) -> np.ndarray:
    return np.array([profile.stats_local_msv_mu, profile.stats_local_msv_lambda, profile.stats_local_viterbi_mu,
                     profile.stats_local_viterbi_lambda, profile.stats_local_forward_theta,
                     profile.stats_local_forward_lambda], np.float32)


_CAL_SETS = ("msv", "viterbi", "forward")


def _cal_triple(value, what: str) -> tuple:
    """n= / length=: None (the defaults), one number for every set, or one per set (MSV, Viterbi, Forward)."""
    if value is None:
        return (0, 0, 0)
    if np.ndim(value) == 0:
        return (int(value),) * 3
    if len(value) != 3:
        raise ValueError(f"{what} is one number or three")
    return tuple(int(v) for v in value)


def _calibrate(call, profile, engines, n, length, tail, seed, workspace_bytes, insert_mode, keep_scores):
    opt = _native.CalOptions(_cal_triple(n, "n"), _cal_triple(length, "length"), tail, seed, insert_mode,
                             workspace_bytes)
    from_file = _file_stats(profile)
    stats = from_file.copy()
    rep = _native.CalReport()
    scores = {}
    if keep_scores:
        for s, name in enumerate(_CAL_SETS):
            if engines[s]:
                scores[name] = np.zeros(opt.n[s] or (200, 200, 200)[s], np.float32)
                opt.scores[s] = scores[name].ctypes.data
    check(call(opt, stats, rep), "calibrate")
    report = rep.as_dict()
    report["lambda"] = report.pop("lambda_")
    return Calibration(stats, rep.lambda_, report, from_file, scores)


def calibrate(profile: Profile_HMM, msv_engine: "MSV_HMM | None" = None, vit_engine: "Viterbi_HMM | None" = None,
              fwd_engine: "Forward_HMM | None" = None, *, n=None, length=None, tail: float = 0.04, seed: int = 42,
              workspace_bytes: int = 0, keep_scores: bool = False) -> Calibration:
    """HMMER3's p7_Calibrate for this library's engines, on the GPU (msv_cal_calibrate): per engine given, a null
    sample of n iid background sequences of `length` residues (defaults 200 x 200, 200 x 200, 200 x 100; one number
    for all three sets or one per set) is generated on the device, scored by the engine and fitted there: the MSV and
    Viterbi mu at the profile's lambda, the Forward tau from a complete Gumbel fit and the tail mass.  An engine that
    is None is skipped and its two slots keep the file's values.  The profile's own statistics are not modified."""
    L = _native.lib()
    engines = (msv_engine, vit_engine, fwd_engine)
    ptrs = [e._p if e is not None else None for e in engines]
    return _calibrate(lambda opt, stats, rep: L.msv_cal_calibrate(profile._h, *ptrs, C.byref(opt), stats.ctypes.data,
                                                                  C.byref(rep)),
                      profile, engines, n, length, tail, seed, workspace_bytes, 0, keep_scores)


def cal_cpu_calibrate(profile: Profile_HMM, sets=_CAL_SETS, *, insert_mode: int = INSERTS_ZERO, n=None, length=None,
                      tail: float = 0.04, seed: int = 42, keep_scores: bool = False) -> Calibration:
    """The CPU twin of calibrate() (msv_cal_cpu_calibrate): the same sample, the CPU DPs, the host fits."""
    L = _native.lib()
    run = tuple(name in sets for name in _CAL_SETS)
    mask = sum(1 << s for s in range(3) if run[s])
    return _calibrate(lambda opt, stats, rep: L.msv_cal_cpu_calibrate(profile._h, mask, C.byref(opt),
                                                                      stats.ctypes.data, C.byref(rep)),
                      profile, run, n, length, tail, seed, 0, insert_mode, keep_scores)


def cal_lambda(profile: Profile_HMM) -> float:
    """The profile's lambda from its match emissions and the background (msv_cal_lambda, HMMER's p7_Lambda)."""
    em = np.ascontiguousarray(profile.match_emissions, np.float32)
    out = C.c_double()
    check(_native.lib().msv_cal_lambda(em.ctypes.data, profile.model_length,
                                       background_frequencies().ctypes.data, C.byref(out)), "msv_cal_lambda")
    return out.value


def cal_thresholds(background=None) -> np.ndarray:
    """The 19 thresholds of the null sample's draw (msv_cal_thresholds) -> uint32[19]."""
    bg = np.ascontiguousarray(background_frequencies() if background is None else background, np.float32)
    out = np.zeros(19, np.uint32)
    check(_native.lib().msv_cal_thresholds(bg.ctypes.data, out.ctypes.data), "msv_cal_thresholds")
    return out


def cal_codes_of_draws(draws, background=None) -> np.ndarray:
    """The residue codes of 24-bit draws (msv_cal_codes_of_draws) -> uint8[n]."""
    bg = np.ascontiguousarray(background_frequencies() if background is None else background, np.float32)
    draws = np.ascontiguousarray(draws, np.uint32)
    out = np.zeros(draws.size, np.uint8)
    check(_native.lib().msv_cal_codes_of_draws(bg.ctypes.data, _ptr(draws), draws.size, _ptr(out)),
          "msv_cal_codes_of_draws")
    return out


def cal_generate(seed: int, set: int, first: int, n: int, length: int, background=None):
    """THE null sample (msv_cal_generate): sequences first .. first + n - 1 of a sample set -> (codes, offsets)."""
    bg = np.ascontiguousarray(background_frequencies() if background is None else background, np.float32)
    codes = np.zeros(n * length, np.uint8)
    offsets = np.zeros(n + 1, np.uint64)
    check(_native.lib().msv_cal_generate(bg.ctypes.data, seed & (2 ** 64 - 1), set, first, n, length, _ptr(codes),
                                         offsets.ctypes.data), "msv_cal_generate")
    return codes, offsets


def cal_fit_location(scores, lam: float, length: int = 0) -> float:
    """mu of a Gumbel of known lambda (msv_cal_fit_location); length = 0: the scores are bit scores already."""
    scores = np.ascontiguousarray(scores, np.float32)
    out = C.c_double()
    check(_native.lib().msv_cal_fit_location(_ptr(scores), scores.size, length, lam, C.byref(out)),
          "msv_cal_fit_location")
    return out.value


def cal_fit_gumbel(scores, length: int = 0):
    """The complete Gumbel fit (msv_cal_fit_gumbel) -> (mu, lambda, Newton iterations)."""
    scores = np.ascontiguousarray(scores, np.float32)
    mu, lam, it = C.c_double(), C.c_double(), C.c_uint32()
    check(_native.lib().msv_cal_fit_gumbel(_ptr(scores), scores.size, length, C.byref(mu), C.byref(lam),
                                           C.byref(it)), "msv_cal_fit_gumbel")
    return mu.value, lam.value, it.value


def cal_tau(gmu: float, glam: float, lam: float, tail: float = 0.04) -> float:
    """Forward's tau from the fitted Gumbel, the profile's lambda and the tail mass (msv_cal_tau, HMMER's p7_Tau)."""
    out = C.c_double()
    check(_native.lib().msv_cal_tau(gmu, glam, lam, tail, C.byref(out)), "msv_cal_tau")
    return out.value


def write_hmm_stats(src_path: str, dst_path: str, stats) -> None:
    """Copies a profile's text with its three STATS LOCAL lines rewritten, in the file's own format, to the given six
    (a Calibration or six floats): a calibrated profile saved for the unchanged parser.  Every other byte is kept."""
    six = _six_stats(stats)
    form = {"MSV": "STATS LOCAL MSV      %8.4f %8.5f", "VITERBI": "STATS LOCAL VITERBI  %8.4f %8.5f",
            "FORWARD": "STATS LOCAL FORWARD  %8.4f %8.5f"}
    slot = {"MSV": 0, "VITERBI": 2, "FORWARD": 4}
    with open(src_path, "r", encoding="latin-1", newline="") as f:
        lines = f.read().split("\n")
    seen = set()
    for i, line in enumerate(lines):
        w = line.split()
        if len(w) >= 3 and w[0] == "STATS" and w[1] == "LOCAL" and w[2] in form and w[2] not in seen:
            seen.add(w[2])
            lines[i] = form[w[2]] % (six[slot[w[2]]], six[slot[w[2]] + 1]) + ("\r" if line.endswith("\r") else "")
        if line.startswith("HMM "):
            break
    if len(seen) != 3:
        raise ValueError(f"{src_path} has no three STATS LOCAL lines")
    with open(dst_path, "w", encoding="latin-1", newline="") as f:
        f.write("\n".join(lines))


class Emitted:
    """What Emitter.emit / cpu_emit return (msv.h "Emit stage"): the CSR batch `codes` uint8 and `offsets`
    uint64 [n + 1], `truncated` bool [n], `traces` -- the true paths as a Traces (domains, ops; scores =
    msv_emit_path_score under the engines' tables), None where truth was not asked for -- and `chunks`, the device
    chunks the call ran (0 for the host definition)."""

    def __init__(self, codes, offsets, truncated, traces, chunks=0):
        self.codes, self.offsets, self.truncated, self.traces, self.chunks = codes, offsets, truncated, traces, chunks

    def __len__(self) -> int:
        return len(self.offsets) - 1

    def sequences(self) -> list[str]:
        """The batch in the reference's form: '#' + one-letter residues."""
        letters = np.frombuffer(AMINO_ACIDS.encode(), np.uint8)[self.codes].tobytes().decode()
        return ["#" + letters[int(self.offsets[i]):int(self.offsets[i + 1])] for i in range(len(self))]


def _emit_take(handle, with_truth: bool):
    """An msv_emit_result as numpy arrays (and frees it) -> (codes, offsets, domain_offsets, domains, ops, truncated,
    chunks)."""
    L = _native.lib()
    try:
        n = int(L.msv_emit_result_count(handle))
        codes = np.zeros(int(L.msv_emit_result_residues(handle)), np.uint8)
        offsets = np.zeros(n + 1, np.uint64)
        dom_off = np.zeros(n + 1, np.uint64)
        doms = np.zeros(int(L.msv_emit_result_domains(handle)) if with_truth else 0, _native.DOMAIN_DTYPE)
        ops = np.zeros(int(L.msv_emit_result_ops(handle)) if with_truth else 0, np.uint8)
        trunc = np.zeros(n, np.uint8)
        check(L.msv_emit_result_copy(handle, _ptr(codes), offsets.ctypes.data, dom_off.ctypes.data, _ptr(doms),
                                     _ptr(ops), _ptr(trunc)), "msv_emit_result_copy")
        return codes, offsets, dom_off, doms, ops, trunc.astype(bool), int(L.msv_emit_result_chunks(handle))
    finally:
        L.msv_emit_result_free(handle)


def emit_tables(profile: Profile_HMM, length: int = 400, multihit: bool = True, insert_mode: int = INSERTS_ZERO,
                max_length: int | None = None) -> dict:
    """The emit stage's integer thresholds (msv_emit_tables): background uint32[19], match and insert [M, 19],
    transitions [M, 4] = (T_MM, T_MM+MI, T_IM, T_DM), specials (T_loop, T_J)."""
    M = profile.model_length
    out = {"background": np.zeros(19, np.uint32), "match": np.zeros((M, 19), np.uint32),
           "insert": np.zeros((M, 19), np.uint32), "transitions": np.zeros((M, 4), np.uint32),
           "specials": np.zeros(2, np.uint32)}
    opt = _native.EmitOptions(length, multihit, insert_mode, max_length)
    check(_native.lib().msv_emit_tables(profile._h, C.byref(opt), *[a.ctypes.data for a in out.values()]),
          "msv_emit_tables")
    return out


def emit_generate(profile: Profile_HMM, n: int, seed: int = 42, first: int = 0, *, length: int = 400,
                  multihit: bool = True, insert_mode: int = INSERTS_ZERO, max_length: int | None = None):
    """THE definition of the emit stage (msv_emit_generate): sequences first .. first + n - 1 drawn from the profile
    -> (codes, offsets, domain_offsets, domains, ops, truncated)."""
    opt = _native.EmitOptions(length, multihit, insert_mode, max_length)
    h = C.c_void_p()
    check(_native.lib().msv_emit_generate(profile._h, C.byref(opt), seed & (2 ** 64 - 1), first, n, C.byref(h)),
          "msv_emit_generate")
    return _emit_take(h, True)[:6]


def emit_path_score(match_scores, insert_scores, transition_scores, consts, codes, domains, ops) -> float:
    """The nats score of a given true path of one sequence (msv_emit_path_score): tables as msv_hmm_viterbi_scores
    gives them (insert_scores None = zeros), consts = (tr_B_Mk, tr_E_C, tr_E_J), `domains` with ops_begin into `ops`."""
    msc = np.ascontiguousarray(match_scores, np.float32)
    isc = None if insert_scores is None else np.ascontiguousarray(insert_scores, np.float32)
    tsc = np.ascontiguousarray(transition_scores, np.float32)
    codes = np.ascontiguousarray(codes, np.uint8)
    domains = np.ascontiguousarray(domains, _native.DOMAIN_DTYPE)
    ops = np.ascontiguousarray(ops, np.uint8)
    out = C.c_double()
    _check_residues(_native.lib().msv_emit_path_score(
        msc.ctypes.data, None if isc is None else isc.ctypes.data, tsc.ctypes.data, msc.shape[1],
        *[float(x) for x in consts], _ptr(codes), codes.size, _ptr(domains), len(domains), _ptr(ops), C.byref(out)),
        "msv_emit_path_score")
    return out.value


class Emitter:
    """Sequences drawn from a profile on the GPU, with the paths that drew them (msv.h "Emit stage"): the
    positive sample, the sibling of calibration's null sample.  It samples THIS library's scoring model run forwards
    -- a fragment uniform over the LENG (LENG + 1) / 2 (k_start, k_end) pairs, not HMMER's occupancy-weighted entry --
    so parity with hmmemit is unpinned.  `length` is the configured length Lc of the flanks (0: none), `multihit`
    E -> J with 1/2, `insert_mode` where insert residues come from (INSERTS_ZERO: the background), `max_length` the
    cut (None: 2^20).  A sequence depends on (seed, index, this configuration) only.  The device handle is made on
    first use; cpu_emit, the definition, needs no GPU."""

    def __init__(self, profile: Profile_HMM, length: int = 400, multihit: bool = True,
                 insert_mode: int = INSERTS_ZERO, max_length: int | None = None, device: int = 0):
        self._profile = profile
        self.length, self.multihit, self.insert_mode, self.max_length = length, multihit, insert_mode, max_length
        self.device = device
        self._opt = _native.EmitOptions(length, multihit, insert_mode, max_length)
        check(_native.lib().msv_emit_tables(profile._h, C.byref(self._opt), None, None, None, None, None),
              "msv_emit_tables")
        self._p = None
        self._score_tables = None

    def _handle(self):
        if self._p is None:
            p = C.c_void_p()
            check(_native.lib().msv_emit_profile_create(self.device, self._profile._h, C.byref(self._opt),
                                                        C.byref(p)), "msv_emit_profile_create")
            self._p = p
        return self._p

    def _tables(self):
        """The engines' tables the true paths are scored under (msv_hmm_viterbi_scores, this emitter's insert mode)."""
        if self._score_tables is None:
            M = self._profile.model_length
            msc, isc, tsc = np.zeros((20, M), np.float32), np.zeros((20, M), np.float32), np.zeros((M, 7), np.float32)
            b, c, j = C.c_float(), C.c_float(), C.c_float()
            check(_native.lib().msv_hmm_viterbi_scores(self._profile._h, self.insert_mode, msc.ctypes.data,
                                                       isc.ctypes.data, tsc.ctypes.data, C.byref(b), C.byref(c),
                                                       C.byref(j)), "msv_hmm_viterbi_scores")
            self._score_tables = (msc, isc if self.insert_mode else None, tsc, (b.value, c.value, j.value))
        return self._score_tables

    def path_scores(self, codes, offsets, domain_offsets, domains, ops) -> np.ndarray:
        """msv_emit_path_score of every sequence of a batch with its truth -> float64 [n] (-inf: no domain)."""
        msc, isc, tsc, consts = self._tables()
        n = len(offsets) - 1
        out = np.zeros(n, np.float64)
        for q in range(n):
            d = domains[int(domain_offsets[q]):int(domain_offsets[q + 1])]
            out[q] = emit_path_score(msc, isc, tsc, consts, codes[int(offsets[q]):int(offsets[q + 1])], d, ops)
        return out

    def _emitted(self, taken, truth: bool, scores: bool) -> Emitted:
        codes, offsets, dom_off, doms, ops, trunc, chunks = taken
        traces = None
        if truth:
            sc = (self.path_scores(codes, offsets, dom_off, doms, ops) if scores
                  else np.full(len(offsets) - 1, np.nan))
            traces = Traces(sc, dom_off, doms, ops, stats={"chunks": chunks}, codes=codes, offsets=offsets)
        return Emitted(codes, offsets, trunc, traces, chunks)

    def cpu_emit(self, n: int, seed: int = 42, first: int = 0, scores: bool = True) -> Emitted:
        """The definition (msv_emit_generate) on the host."""
        h = C.c_void_p()
        check(_native.lib().msv_emit_generate(self._profile._h, C.byref(self._opt), seed & (2 ** 64 - 1), first, n,
                                              C.byref(h)), "msv_emit_generate")
        return self._emitted(_emit_take(h, True), True, scores)

    def emit(self, n: int, seed: int = 42, first: int = 0, truth: bool = True, workspace_bytes: int = 0,
             stream: int | None = None, scores: bool = True) -> Emitted:
        """Sequences first .. first + n - 1 on the GPU, downloaded (msv_emit_batch): in chunks that fit
        workspace_bytes (0: 256 MiB); the bytes do not depend on the chunking and equal cpu_emit's.  scores=False
        leaves the traces' scores NaN (msv_emit_path_score runs on the host, once per sequence)."""
        h = C.c_void_p()
        check(_native.lib().msv_emit_batch(self._handle(), seed & (2 ** 64 - 1), first, n, 1 if truth else 0,
                                           workspace_bytes, stream, C.byref(h)), "msv_emit_batch")
        return self._emitted(_emit_take(h, truth), truth, scores)

    @staticmethod
    def workspace_bytes(n: int, residues: int, domains: int, ops: int, truth: bool = True) -> int:
        """Device bytes of one chunk holding these totals (msv_emit_workspace_bytes)."""
        return int(_native.lib().msv_emit_workspace_bytes(n, residues, domains, ops, 1 if truth else 0))

    def emit_into(self, n: int, codes_ptr: int, capacity: int, offsets_ptr: int, *, seed: int = 42, first: int = 0,
                  truth: "_native.EmitTruth | None" = None, stream: int) -> dict:
        """msv_emit_batch_device into the caller's device buffers (raw pointers), on `stream`; returns the totals
        record.  MSVError MSV_ERR_OUT_OF_MEMORY (its .totals set) where a total exceeds its capacity: nothing was
        written."""
        tot = _native.EmitTotals()
        st = _native.lib().msv_emit_batch_device(self._handle(), seed & (2 ** 64 - 1), first, n, codes_ptr, capacity,
                                                 offsets_ptr, C.byref(truth) if truth is not None else None,
                                                 C.byref(tot), stream)
        if st != _native.MSV_OK:
            err = MSVError(st, "msv_emit_batch_device")
            err.totals = tot.as_dict()
            raise err
        return tot.as_dict()

    def emit_device(self, n: int, seed: int = 42, first: int = 0, truth: bool = True,
                    stream: int | None = None) -> dict:
        """The batch left on the device for chaining into the engines' *_device calls: torch tensors sized by a first
        call that only counts (capacity 0), then the call itself.  Returns the tensors (codes, offsets and, with truth,
        domain_offsets, domains as raw bytes, ops, truncated), their pointers (codes_ptr, residues_len, offsets_ptr)
        and the totals.  Needs torch."""
        import torch
        dev = torch.device(f"cuda:{self.device}")
        st = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
        d_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        d_doff = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        d_trunc = torch.zeros(max(n, 1), dtype=torch.uint8, device=dev)
        t = _native.EmitTruth(d_doff.data_ptr(), None, 0, None, 0, d_trunc.data_ptr()) if truth else None
        torch.cuda.synchronize(dev)
        try:
            tot = self.emit_into(n, None, 0, d_off.data_ptr(), seed=seed, first=first, truth=t, stream=st)
        except MSVError as e:
            if e.name != "MSV_ERR_OUT_OF_MEMORY" or e.totals["residues"] >= (1 << 32) - (1 << 20):
                raise
            tot = e.totals
        d_codes = torch.zeros(max(tot["residues"], 1), dtype=torch.uint8, device=dev)
        out = {"codes": d_codes, "offsets": d_off}
        if truth:
            d_doms = torch.zeros(max(tot["domains"], 1) * 32, dtype=torch.uint8, device=dev)
            d_ops = torch.zeros(max(tot["ops"], 1), dtype=torch.uint8, device=dev)
            t = _native.EmitTruth(d_doff.data_ptr(), d_doms.data_ptr(), tot["domains"], d_ops.data_ptr(), tot["ops"],
                                  d_trunc.data_ptr())
            out.update(domain_offsets=d_doff, domains=d_doms, ops=d_ops, truncated=d_trunc[:n])
        torch.cuda.synchronize(dev)
        out["totals"] = self.emit_into(n, d_codes.data_ptr(), tot["residues"], d_off.data_ptr(), seed=seed,
                                       first=first, truth=t, stream=st)
        out.update(n=n, codes_ptr=d_codes.data_ptr(), residues_len=tot["residues"], offsets_ptr=d_off.data_ptr())
        return out

    def last_times(self) -> dict:
        """Device times in ms of the last emit / emit_into call's count, scan and place launches (HIP events)."""
        c, s, p = C.c_float(), C.c_float(), C.c_float()
        check(_native.lib().msv_emit_profile_times(self._handle(), C.byref(c), C.byref(s), C.byref(p)),
              "msv_emit_profile_times")
        return {"count_ms": c.value, "scan_ms": s.value, "place_ms": p.value}

    def bind_stream(self, stream: int | None) -> None:
        """msv_emit_profile_bind_stream: emit()'s working stream where none is given (None: the handle's own)."""
        check(_native.lib().msv_emit_profile_bind_stream(self._handle(), stream), "msv_emit_profile_bind_stream")

    def describe(self) -> dict:
        info = _native.EmitInfo()
        check(_native.lib().msv_emit_describe(self._handle(), C.byref(info)), "msv_emit_describe")
        return info.as_dict()

    def close(self):
        lib = _loaded_lib()
        if getattr(self, "_p", None) and lib is not None:
            lib.msv_emit_profile_destroy(self._p)
            self._p = None

    def __del__(self):
        self.close()


def search_pipeline(msv_engine: MSV_HMM, vit_engine: Viterbi_HMM, fwd_engine: Forward_HMM,
                    seqs: Sequence[str] | None = None, *, codes: np.ndarray | None = None,
                    offsets: np.ndarray | None = None, F1: float = 0.02, F2: float = 1e-3,
                    dom_engine: "Domain_HMM | None" = None, F3: float = 1e-5, align: bool = False,
                    null2: bool = False, bias_engine: "Bias_filter | None" = None, split: bool = False,
                    stats=None) -> dict:
    """HMMER3's whole cascade on the GPU (msv_fwd_filter_batch): MSV over every sequence, P <= F1, Viterbi on the
    survivors, P <= F2, Forward on those, Forward P-values.  Returns the per-stage arrays: msv_scores, passed_msv,
    vit_scores (-inf where not run), passed_vit, fwd_scores (-inf where not run), fwd_pvalues (1 where not run).
    With dom_engine, also "envelopes": the Envelopes of the sequences with Forward P <= F3, in index order (a second
    call that uploads the batch again: Domain_HMM.decode_batch with select = those indices).  With align=True (which
    needs dom_engine) also "alignments": Domain_HMM.align_batch of every region of those envelopes.  With null2=True
    (which needs align=True) the alignments carry null2 (msv.h "Bias stage") and the dict gains domain_bits,
    domain_pvalues (per alignment item) and seq_bias, seq_bits, seq_pvalues, indexed as the envelopes' sequences are
    (entry q is sequence envelopes.select[q]).
    With bias_engine (a Bias_filter: msv.h "Bias filter", HMMER3's composition filter, on by default in hmmsearch) the
    call is msv_fwd_filter_batch_opts: the MSV survivors (passed_msv) are scored by the bias filter, only those whose
    filtered MSV P-value is still <= F1 (passed_bias) reach Viterbi, the Viterbi and Forward tests and fwd_pvalues
    use the filtered bit score, and the dict gains "bias" (float32 [n], 0 where not run) and "passed_bias"; the
    dom_engine hit selection uses the filtered fwd_pvalues, as HMMER3's F3 test does; null2's reporting is against
    null1 and null2, as HMMER3's, and does not change.
    With split=True (which needs align=True; msv.h "Split stage") the regions are first put through
    Domain_HMM.split_regions: a multi-domain region is sampled and clustered, "alignments" holds one item per cluster
    envelope in place of the region, and the dict gains "split" (split_regions' dict: which region each item came
    from and its prob).  With split=False no launch or allocation is added and every returned byte is unchanged.
    stats (a Calibration, e.g. calibrate()'s, or six floats in msv_hmm_stats' order) takes the place of the engines'
    file values everywhere they go: the three tests, fwd_pvalues and null2's bias_scores.  With stats=None no byte of
    any result changes and no launch is added."""
    if null2 and not align:
        raise ValueError("null2=True needs align=True")
    if split and not align:
        raise ValueError("split=True needs align=True")
    codes, offsets, n = _batch(seqs, codes, offsets)
    if stats is None:
        stats = np.array([msv_engine.msv_mu, msv_engine.msv_lambda, vit_engine.viterbi_mu, vit_engine.viterbi_lambda,
                          fwd_engine.forward_tau, fwd_engine.forward_lambda], np.float32)
    else:
        stats = np.array(_six_stats(stats), np.float32)
    msc, vsc, fsc = (np.zeros(n, np.float32) for _ in range(3))
    p1, p2 = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    fpv = np.zeros(n, np.float64)
    n1, n2 = C.c_uint64(0), C.c_uint64(0)
    if bias_engine is None:
        _check_residues(_native.lib().msv_fwd_filter_batch(
            msv_engine._p, vit_engine._p, fwd_engine._p, _ptr(codes), offsets.ctypes.data, n, stats.ctypes.data, F1,
            F2, msc.ctypes.data, p1.ctypes.data, vsc.ctypes.data, p2.ctypes.data, fsc.ctypes.data, fpv.ctypes.data,
            C.byref(n1), C.byref(n2)), "msv_fwd_filter_batch")
    else:
        bias, pb, nb = np.zeros(n, np.float32), np.zeros(n, np.uint8), C.c_uint64(0)
        opt = _native.SearchOptions(C.sizeof(_native.SearchOptions), 1, 0, bias_engine._p)
        _check_residues(_native.lib().msv_fwd_filter_batch_opts(
            msv_engine._p, vit_engine._p, fwd_engine._p, _ptr(codes), offsets.ctypes.data, n, stats.ctypes.data, F1,
            F2, C.byref(opt), msc.ctypes.data, p1.ctypes.data, vsc.ctypes.data, p2.ctypes.data, fsc.ctypes.data,
            fpv.ctypes.data, C.byref(n1), C.byref(n2), bias.ctypes.data, pb.ctypes.data, C.byref(nb)),
            "msv_fwd_filter_batch_opts")
    out = {"msv_scores": msc, "passed_msv": p1.astype(bool), "vit_scores": vsc, "passed_vit": p2.astype(bool),
           "fwd_scores": fsc, "fwd_pvalues": fpv}
    if bias_engine is not None:
        out["bias"], out["passed_bias"] = bias, pb.astype(bool)
    if dom_engine is not None:
        hits = np.flatnonzero(p2.astype(bool) & (fpv <= F3)).astype(np.uint32)
        out["envelopes"] = dom_engine.decode_batch(codes=codes, offsets=offsets, select=hits)
        if align:
            if split:
                out["split"] = dom_engine.split_regions(out["envelopes"], codes=codes, offsets=offsets)
                out["alignments"] = dom_engine.align_batch(codes=codes, offsets=offsets, items=out["split"]["items"],
                                                           null2=null2)
            else:
                out["alignments"] = dom_engine.align_batch(codes=codes, offsets=offsets,
                                                           envelopes=out["envelopes"], null2=null2)
            if null2:
                b = out["alignments"].bias_scores(float(stats[4]), float(stats[5]), fwd_scores=fsc)
                out["domain_bits"], out["domain_pvalues"] = b["domain_bits"], b["domain_pvalues"]
                for k in ("seq_bias", "seq_bits", "seq_pvalues"):
                    out[k] = b[k][hits]
    elif align:
        raise ValueError("align=True needs dom_engine")
    return out


def _handles(engines: Sequence[MSV_HMM]):
    arr = (C.c_void_p * len(engines))(*[e._p for e in engines])
    return arr


def score_grid(engines: Sequence[MSV_HMM], seqs: Sequence[str] | None = None, *, codes: np.ndarray | None = None,
               offsets: np.ndarray | None = None, out: np.ndarray | None = None) -> np.ndarray:
    """Profiles x sequences grid -> float32 [len(engines), n]: the reference's
    benchmark loop over every profile for one FASTA set (benchmark_MSV.cpp:12-24,31-41), as one
    host call: one upload, one longest-first order, then ONE fused launch over all profiles for a
    few sequences, else one launch per profile forked onto the profiles' own streams.  `out`: an
    optional C-contiguous float32 [len(engines), n] destination (page-locked, e.g. pinned_empty,
    is written by the kernels directly); page-locked `codes` are read in place."""
    if not engines:
        raise ValueError("score_grid needs at least one profile")
    codes, offsets, n = _batch(seqs, codes, offsets)
    if out is None:
        out = np.zeros((len(engines), n), np.float32)
    elif out.dtype != np.float32 or out.shape != (len(engines), n) or not out.flags.c_contiguous:
        raise ValueError("out must be a C-contiguous float32 array of shape (len(engines), n)")
    _check_residues(_native.lib().msv_score_grid(_handles(engines), len(engines), _ptr(codes), offsets.ctypes.data, n,
                                                 out.ctypes.data, None), "msv_score_grid")
    return out


def score_grid_device(engines: Sequence[MSV_HMM], residues_ptr: int, residues_len: int, offsets_ptr: int, n: int,
                      scores_ptr: int, order_ptr: int | None = None, stream: int | None = None) -> None:
    """Device-resident grid: scores_ptr -> float32 [len(engines)][n]; async on `stream`; errors via
    each engine's check()."""
    check(_native.lib().msv_score_grid_device(_handles(engines), len(engines), residues_ptr, residues_len,
                                              offsets_ptr, n, order_ptr, scores_ptr, stream), "msv_score_grid_device")


def shard_bounds(offsets: np.ndarray, n_shards: int) -> np.ndarray:
    """uint64[n_shards + 1] contiguous, residue-balanced shard boundaries (msv_shard_bounds)."""
    offsets = np.ascontiguousarray(offsets, np.uint64)
    out = np.zeros(n_shards + 1, np.uint64)
    check(_native.lib().msv_shard_bounds(offsets.ctypes.data, len(offsets) - 1, n_shards, out.ctypes.data),
          "msv_shard_bounds")
    return out


def score_batch_multi(engines: Sequence[MSV_HMM], seqs: Sequence[str] | None = None, *,
                      codes: np.ndarray | None = None, offsets: np.ndarray | None = None) -> np.ndarray:
    """One batch over several devices from this one process (engines[k] = the profile on device k):
    residue-balanced contiguous shards scored concurrently, scores in input order."""
    if not engines:
        raise ValueError("score_batch_multi needs at least one engine")
    codes, offsets, n = _batch(seqs, codes, offsets)
    out = np.zeros(n, np.float32)
    _check_residues(_native.lib().msv_score_batch_multi(_handles(engines), len(engines), _ptr(codes),
                                                        offsets.ctypes.data, n, out.ctypes.data),
                    "msv_score_batch_multi")
    return out


class MultiGPU:
    """One batch over several GPUs from this process, scores gathered over RCCL (msv_multi_*):
    engines[k] = the same model on DISTINCT devices; residue-balanced shards, one grouped RCCL
    send/recv into device 0, one D2H."""

    def __init__(self, engines: Sequence[MSV_HMM]):
        if not engines:
            raise ValueError("MultiGPU needs at least one engine")
        self._engines = list(engines)  # the context refers to their profiles
        m = C.c_void_p()
        check(_native.lib().msv_multi_create(_handles(self._engines), len(self._engines), C.byref(m)),
              "msv_multi_create")
        self._m = m

    def score_batch(self, seqs: Sequence[str] | None = None, *, codes: np.ndarray | None = None,
                    offsets: np.ndarray | None = None) -> np.ndarray:
        codes, offsets, n = _batch(seqs, codes, offsets)
        out = np.zeros(n, np.float32)
        _check_residues(_native.lib().msv_multi_score_batch(self._m, _ptr(codes), offsets.ctypes.data, n,
                                                            out.ctypes.data), "msv_multi_score_batch")
        return out

    def close(self):
        lib = _loaded_lib()
        if getattr(self, "_m", None) and lib is not None:
            lib.msv_multi_destroy(self._m)
            self._m = None

    def __del__(self):
        self.close()


class FASTA_device:
    """FASTA parsed on the GPU (msv_fasta_read_device / msv_fasta_parse_device): the
    same records as FASTA_protein_sequences, left in device memory as the scorer's CSR input.
    `codes_ptr`/`offsets_ptr` feed MSV_HMM.score_batch_device directly."""

    def __init__(self, path: str | None = None, *, text_ptr: int | None = None, n: int = 0, device: int = 0,
                 stream: int | None = None):
        L = _native.lib()
        f = C.c_void_p()
        if path is not None:
            check(L.msv_fasta_read_device(device, str(path).encode(), stream, C.byref(f)), f"FASTA_device({path})")
        else:
            check(L.msv_fasta_parse_device(device, text_ptr, n, stream, C.byref(f)), "msv_fasta_parse_device")
        self._f = f
        self.device = device
        self.count = int(L.msv_fasta_device_count(f))
        self.rejected = int(L.msv_fasta_device_rejected(f))
        self.residues = int(L.msv_fasta_device_residues(f))
        self.max_length = int(L.msv_fasta_device_max_length(f))
        self.codes_ptr = L.msv_fasta_device_codes(f)
        self.offsets_ptr = L.msv_fasta_device_offsets(f)
        self.spans_ptr = L.msv_fasta_device_header_spans(f)

    def download(self):
        """(codes uint8, offsets uint64[count+1], spans uint64[count, 2]) on the host."""
        codes = np.zeros(self.residues, np.uint8)
        offsets = np.zeros(self.count + 1, np.uint64)
        spans = np.zeros((self.count, 2), np.uint64)
        check(_native.lib().msv_fasta_device_download(self._f, codes.ctypes.data if self.residues else None,
                                                      offsets.ctypes.data, spans.ctypes.data if self.count else None),
              "msv_fasta_device_download")
        return codes, offsets, spans

    def close(self):
        lib = _loaded_lib()
        if getattr(self, "_f", None) and lib is not None:
            lib.msv_fasta_device_destroy(self._f)
            self._f = None

    def __del__(self):
        self.close()

    def __len__(self):
        return self.count
