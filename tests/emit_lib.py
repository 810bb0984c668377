"""Shared by the emit stage's tests: tiny profiles written as HMMER3 text from given probabilities, the model's
probability of an emitted outcome as a plain product in Python floats (independent of the C code), an enumeration of
every outcome above a cutoff, and the outcomes of an emitted batch read from its truth."""
import math
import os

import numpy as np

import hmm_fasta_viterbi_amd as msv

AMINO = msv.AMINO_ACIDS
DATA = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "data", "profile_HMMs")
MM, MI, MD, IM, II, DM, DD = range(7)


def _field(p: float) -> str:
    return "  200.00000" if p <= 0.0 else f"  {-math.log(p):9.7f}"


def write_tiny_hmm(path: str, match, insert, trans) -> None:
    """A profile of LENG = len(match) from probabilities: match / insert [LENG][20], trans [LENG][7] (file order; the
    last node's are not read by any stage).  A probability 0 is written as 200 (exp(-200) is 0 in float32)."""
    leng = len(match)
    out = ["HMMER3/b [tiny]", f"NAME  tiny_{leng}", f"LENG  {leng}", "ALPH  amino",
           "STATS LOCAL MSV       -9.9000  0.70000", "STATS LOCAL VITERBI  -10.5000  0.70000",
           "STATS LOCAL FORWARD   -4.0000  0.70000", "HMM     " + "".join(f"     {a}   " for a in AMINO),
           "            m->m     m->i     m->d     i->m     i->i     d->m     d->d"]
    flat = "".join(_field(0.05) for _ in range(20))
    out += ["  COMPO " + flat, "        " + flat,
            "        " + "".join(_field(p) for p in (0.9, 0.05, 0.05, 0.5, 0.5, 1.0, 1.0))]
    for k in range(leng):
        out.append(f"{k + 1:7d} " + "".join(_field(p) for p in match[k]))
        out.append("        " + "".join(_field(p) for p in insert[k]))
        out.append("        " + "".join(_field(p) for p in trans[k]))
    out.append("//")
    with open(path, "w") as f:
        f.write("\n".join(out) + "\n")


def sparse_row(pairs) -> list:
    """A 20-residue row that is zero outside the given (residue, probability) pairs."""
    row = [0.0] * 20
    for r, p in pairs:
        row[r] = p
    return row


class Model:
    """The parsed probabilities of a profile as float64, normalised per group as the emit stage's thresholds are
    (msv.h "Emit stage"), with its configuration."""

    def __init__(self, profile, Lc: int, multihit: bool, insert_mode: int):
        self.leng = profile.model_length - 1
        bg = msv.background_frequencies().astype(np.float64)
        self.bg = bg / bg.sum()
        mat = profile.match_emissions.astype(np.float64)
        self.mat = mat / np.maximum(mat.sum(axis=1, keepdims=True), 1e-300)
        ins = profile.insert_emissions.astype(np.float64)
        self.ins = (ins / np.maximum(ins.sum(axis=1, keepdims=True), 1e-300) if insert_mode
                    else np.tile(self.bg, (len(mat), 1)))
        t = profile.transitions.astype(np.float64)
        self.tm = t[:, [MM, MI, MD]] / np.maximum(t[:, [MM, MI, MD]].sum(axis=1, keepdims=True), 1e-300)
        self.ti = t[:, [IM, II]] / np.maximum(t[:, [IM, II]].sum(axis=1, keepdims=True), 1e-300)
        self.td = t[:, [DM, DD]] / np.maximum(t[:, [DM, DD]].sum(axis=1, keepdims=True), 1e-300)
        self.loop, self.move = Lc / (Lc + 3.0), 3.0 / (Lc + 3.0)
        self.multihit = multihit
        self.npairs = self.leng * (self.leng + 1) // 2

    def step(self, prev: str, op: str, k: int) -> float:
        """The probability of the transition out of state `prev` at node k into `op`."""
        if prev == "M":
            return self.tm[k, "MID".index(op)]
        if prev == "I":
            return self.ti[k, "MI".index(op)] if op in "MI" else 0.0
        return self.td[k, "MD".index(op)] if op in "MD" else 0.0

    def outcome_prob(self, outcome):
        """(probability, draws) of an outcome (flanks, domains): flanks a tuple of residue tuples, one more than the
        domains; a domain (k_from, ops, residues)."""
        flanks, domains = outcome
        p, draws = 1.0, 0
        for f in flanks:
            p *= self.loop ** len(f) * self.move
            draws += 2 * len(f) + 1
            for r in f:
                p *= self.bg[r]
        if not self.multihit and len(domains) != 1:
            return 0.0, draws
        for x, (k_from, ops, res) in enumerate(domains):
            p *= 1.0 / self.npairs
            draws += 1
            k, prev, at = k_from - 1, "", 0
            for op in ops:
                if prev:
                    p *= self.step(prev, op, k)
                    draws += 1
                if op == "M":
                    k += 1
                    p *= self.mat[k, res[at]]
                elif op == "I":
                    p *= self.ins[k, res[at]]
                else:
                    k += 1
                if op != "D":
                    at += 1
                    draws += 1
                prev = op
            if prev == "I" or k > self.leng or at != len(res):
                return 0.0, draws
            if self.multihit:
                p *= 0.5
                draws += 1
        return p, draws

    def enumerate(self, cutoff: float):
        """Every outcome of probability >= cutoff -> {outcome: probability}, by walking the model forwards."""
        out = {}

        def flank(p, then):
            # residues of one flank, then `then(p, flank)`
            def more(p, f):
                if p * self.move >= cutoff:
                    then(p * self.move, f)
                if p * self.loop >= cutoff:
                    for r in range(20):
                        if p * self.loop * self.bg[r] >= cutoff:
                            more(p * self.loop * self.bg[r], f + (r,))
            more(p, ())

        def core(p, k, k_end, st, ops, res, then):
            if st == "M":
                for r in np.flatnonzero(self.mat[k] * p >= cutoff):
                    after(p * self.mat[k, r], k, k_end, "M", ops + "M", res + (int(r),), then)
            elif st == "I":
                for r in np.flatnonzero(self.ins[k] * p >= cutoff):
                    after(p * self.ins[k, r], k, k_end, "I", ops + "I", res + (int(r),), then)
            else:
                after(p, k, k_end, "D", ops + "D", res, then)

        def after(p, k, k_end, st, ops, res, then):
            if st != "I" and k == k_end:
                then(p, ops, res)
                return
            for nxt in "MID":
                q = p * self.step(st, nxt, k)
                if q >= cutoff:
                    core(q, k if nxt == "I" else k + 1, k_end, nxt, ops, res, then)

        def domain(p, flanks, domains):
            for ks in range(1, self.leng + 1):
                for ke in range(ks, self.leng + 1):
                    q = p / self.npairs
                    if q < cutoff:
                        continue

                    def closed(q2, ops, res, ks=ks):
                        doms = domains + ((ks, ops, res),)
                        if self.multihit:
                            flank(q2 * 0.5, lambda q3, f: domain(q3, flanks + (f,), doms))
                            flank(q2 * 0.5, lambda q3, f: out.__setitem__((flanks + (f,), doms), q3))
                        else:
                            flank(q2, lambda q3, f: out.__setitem__((flanks + (f,), doms), q3))
                    core(q, ks, ke, "M", "", (), closed)

        flank(1.0, lambda p, f: domain(p, (f,), ()))
        return out


def outcomes_of(codes, offsets, dom_off, doms, ops):
    """The outcome of every sequence of an emitted batch, from its truth."""
    out = []
    for q in range(len(offsets) - 1):
        seq = codes[int(offsets[q]):int(offsets[q + 1])]
        flanks, domains, at = [], [], 0
        for d in doms[int(dom_off[q]):int(dom_off[q + 1])]:
            flanks.append(tuple(int(x) for x in seq[at:int(d["i_from"]) - 1]))
            o = ops[int(d["ops_begin"]):int(d["ops_begin"]) + int(d["ops_len"])].tobytes().decode()
            domains.append((int(d["k_from"]), o, tuple(int(x) for x in seq[int(d["i_from"]) - 1:int(d["i_to"])])))
            at = int(d["i_to"])
        flanks.append(tuple(int(x) for x in seq[at:]))
        out.append((tuple(flanks), tuple(domains)))
    return out


def replay(d, ops):
    """(i, k) after the ops of domain d, from (i_from - 1, k_from - 1)."""
    o = ops[int(d["ops_begin"]):int(d["ops_begin"]) + int(d["ops_len"])]
    return (int(d["i_from"]) - 1 + int(np.count_nonzero(o != ord("D"))),
            int(d["k_from"]) - 1 + int(np.count_nonzero(o != ord("I"))))


def tiny_profile(tmp_path, leng: int, kind: str = "plain"):
    """A tiny profile with emissions on three residues per match row and two per insert row (every other residue has
    probability 0): `plain`; `closed` (node 1's M -> I closed); `loopy` (tII = 0.9); `nodelete` (node 1's tMD = 0)."""
    match = [sparse_row([(k, 0.5), (k + 5, 0.3), (k + 10, 0.2)]) for k in range(leng)]
    insert = [sparse_row([(17, 0.6), (18, 0.4)]) for _ in range(leng)]
    trans = [[0.7, 0.1, 0.2, 0.6, 0.4, 0.7, 0.3] for _ in range(leng)]
    if kind == "closed":
        trans[0][:3] = [0.8, 0.0, 0.2]
    elif kind == "loopy":
        for t in trans:
            t[3:5] = [0.1, 0.9]
    elif kind == "nodelete":
        trans[0][:3] = [0.9, 0.1, 0.0]
    path = os.path.join(str(tmp_path), f"tiny_{leng}_{kind}.hmm")
    write_tiny_hmm(path, match, insert, trans)
    return msv.Profile_HMM(path)


def op_coordinates(doms, ops):
    """Per op byte of a batch: (domain index, i, k) after the op, vectorised."""
    n_ops = doms["ops_len"].astype(np.int64)
    dom = np.repeat(np.arange(len(doms)), n_ops)
    res = (ops != ord("D")).astype(np.int64)
    node = (ops != ord("I")).astype(np.int64)
    begin = doms["ops_begin"].astype(np.int64)
    cr, cn = np.cumsum(res), np.cumsum(node)
    before_r = np.concatenate([[0], cr])[begin]
    before_n = np.concatenate([[0], cn])[begin]
    i = doms["i_from"].astype(np.int64)[dom] - 1 + cr - before_r[dom]
    k = doms["k_from"].astype(np.int64)[dom] - 1 + cn - before_n[dom]
    return dom, i, k
