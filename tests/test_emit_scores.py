"""The generator and the scorers share one model (msv.h "Emit stage").  For every emitted sequence the
serial Viterbi (msv_vit_cpu_score, float32) is at least the score of the true path (msv_emit_path_score, float64 sums
of the same float32 tables), and the float64 Forward (msv_fwd_cpu_score) at least the Viterbi score.

The tolerance is derived, not fitted: terms 2^-24 max|partial sum|.  The float32 DP holds, for any one path, that
path's score summed in float32 in path order (rounding is monotone, so a max over paths is never below it); n additions
of rounded terms leave that sum within n 2^-24 max|partial sum| of the exact one.  The test rebuilds the path term by
term in path order (_path_terms: one term per flank residue, special, transition and emission, counted exactly; their
float64 sum is checked against msv_emit_path_score) and takes the largest |partial sum|.  Viterbi against the true path
uses the true path's terms; Forward against Viterbi those of Viterbi's own optimal path (msv_vit_cpu_trace)."""
import ctypes as C

import numpy as np
import pytest

import hmm_fasta_viterbi_amd as msv
from hmm_fasta_viterbi_amd import _native
from emit_lib import DATA, tiny_profile


def _tables(profile, insert_mode):
    e = msv.Emitter(profile, insert_mode=insert_mode)
    return e._tables()


def _path_terms(tables, codes, doms, ops):
    """The terms of a path's score in path order, as the DP adds them: per flank residue the loop, the move into B,
    tr_B_Mk, then per core state its transition (but for the first M) and its emission (an insert's only where insert
    scores exist: the DP adds none otherwise), tr_E_J or tr_E_C, and at the end C's move."""
    msc, isc, tsc, (tbm, tec, tej) = tables
    L, nd = len(codes), len(doms)
    loop, move = msv.sequence_transitions(L)
    MM, MI, MD, IM, II, DM, DD = range(7)
    into = {("M", "M"): MM, ("M", "I"): MI, ("M", "D"): MD, ("I", "M"): IM, ("I", "I"): II, ("D", "M"): DM,
            ("D", "D"): DD}
    terms, at = [], 0
    for x, d in enumerate(doms):
        terms += [loop] * (int(d["i_from"]) - 1 - at) + [move, tbm]
        i, k, prev = int(d["i_from"]) - 1, int(d["k_from"]) - 1, ""
        for op in ops[int(d["ops_begin"]):int(d["ops_begin"]) + int(d["ops_len"])].tobytes().decode():
            if prev:
                # a transition is read at the node it leaves: k for M -> I and I -> I, else the node before the new one
                terms.append(float(tsc[k, into[prev, op]]))
            if op == "M":
                i, k = i + 1, k + 1
                terms.append(float(msc[codes[i - 1], k]))
            elif op == "I":
                i += 1
                if isc is not None:
                    terms.append(float(isc[codes[i - 1], k]))
            else:
                k += 1
            prev = op
        terms.append(tej if x + 1 < nd else tec)
        at = int(d["i_to"])
    terms += [loop] * (L - at) + [move]
    return terms


def _path_bound(tables, codes, doms, ops):
    """(terms on the path, the largest |partial sum| of them in path order, their float64 sum)."""
    terms = np.array(_path_terms(tables, codes, doms, ops), np.float64)
    partial = np.cumsum(terms)
    return len(terms), float(np.max(np.abs(partial))), float(partial[-1])


def _check(profile, insert_mode, batch, what):
    codes, off, doff, doms, ops, trunc = batch
    tables = _tables(profile, insert_mode)
    msc, isc, tsc, consts = tables
    lib = _native.lib()
    isc_ptr = None if isc is None else isc.ctypes.data
    worst_v = worst_f = -np.inf
    n = len(off) - 1
    for q in range(n):
        c = np.ascontiguousarray(codes[int(off[q]):int(off[q + 1])])
        d = doms[int(doff[q]):int(doff[q + 1])]
        true = msv.emit_path_score(msc, isc, tsc, consts, c, d, ops)
        assert np.isfinite(true)
        v = C.c_float()
        assert lib.msv_vit_cpu_score(msc.ctypes.data, isc_ptr, tsc.ctypes.data, msc.shape[1], *consts, c.ctypes.data,
                                     c.size, C.byref(v)) == 0
        terms, largest, total = _path_bound(tables, c, d, ops)
        assert abs(total - true) <= 1e-12 * max(1.0, abs(true)), (what, q, total, true)  # the terms ARE the path
        tol = terms * 2.0 ** -24 * largest
        assert v.value >= true - tol, (what, q, v.value, true, tol)
        worst_v = max(worst_v, (true - v.value) / tol)
        f = C.c_double()
        assert lib.msv_fwd_cpu_score(msc.ctypes.data, isc_ptr, tsc.ctypes.data, msc.shape[1], *consts, c.ctypes.data,
                                     c.size, C.byref(f)) == 0
        st, vs, vd, vo = msv._cpu_trace(msc, isc, tsc, consts, c)
        assert st == 0 and np.float32(vs) == np.float32(v.value)
        terms, largest, _ = _path_bound(tables, c, vd, vo)
        tol = terms * 2.0 ** -24 * largest
        assert f.value >= v.value - tol, (what, q, f.value, v.value, tol)
        worst_f = max(worst_f, (v.value - f.value) / tol)
    print(f"emit scores {what}: {n} sequences, worst (true - Viterbi) / tol = {worst_v:.3f}, "
          f"worst (Viterbi - Forward) / tol = {worst_f:.3f}")
    return ops


@pytest.mark.parametrize("insert_mode", [msv.INSERTS_ZERO, msv.INSERTS_LOG_ODDS])
@pytest.mark.parametrize("leng,kind", [(1, "plain"), (2, "plain"), (3, "loopy"), (3, "nodelete")])
def test_tiny_models(tmp_path, leng, kind, insert_mode):
    profile = tiny_profile(tmp_path, leng, kind)
    for Lc, multihit in ((0, False), (2, True)):
        batch = msv.emit_generate(profile, 150, 31 + leng, length=Lc, multihit=multihit, insert_mode=insert_mode)
        _check(profile, insert_mode, batch, f"LENG {leng} {kind} Lc {Lc} inserts {insert_mode}")


@pytest.mark.parametrize("insert_mode", [msv.INSERTS_ZERO, msv.INSERTS_LOG_ODDS])
def test_100_hmm(insert_mode):
    profile = msv.Profile_HMM(f"{DATA}/100.hmm")
    batch = msv.emit_generate(profile, 250, 42, insert_mode=insert_mode)
    ops = _check(profile, insert_mode, batch, f"100.hmm inserts {insert_mode}")
    n_i, n_d = int(np.count_nonzero(ops == ord("I"))), int(np.count_nonzero(ops == ord("D")))
    print(f"emit scores 100.hmm: {n_i} I and {n_d} D ops on the true paths")
    assert n_i > 0 and n_d > 0


def test_emitter_traces_carry_the_path_scores():
    profile = msv.Profile_HMM(f"{DATA}/100.hmm")
    e = msv.Emitter(profile, length=30)
    got = e.cpu_emit(20, seed=3)
    tables = e._tables()
    for q in range(20):
        c = got.codes[int(got.offsets[q]):int(got.offsets[q + 1])]
        want = msv.emit_path_score(*tables[:3], tables[3], c, got.traces.domains_of(q), got.traces.ops)
        assert got.traces.scores[q] == want
    assert got.sequences()[0] == "#" + "".join(msv.AMINO_ACIDS[x] for x in got.codes[:int(got.offsets[1])])
    # a path that does not replay is refused; a sequence without domains has no path in the scoring model
    d = got.traces.domains_of(0).copy()
    d["k_to"][0] += 1
    with pytest.raises(msv.MSVError):
        msv.emit_path_score(*tables[:3], tables[3], got.codes[:int(got.offsets[1])], d, got.traces.ops)
    none = msv.emit_path_score(*tables[:3], tables[3], got.codes[:5], d[:0], got.traces.ops)
    assert none == -np.inf
