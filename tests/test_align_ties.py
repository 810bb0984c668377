"""The twelve tie-breaks of the optimal-accuracy alignment (msv.h "Alignment stage"), in the manner of trace_ties.py:
hand-made float32 posterior arrays on which two candidates of one cell are bitwise equal by construction (small
dyadic numbers, every add exact), the cell on the best path.  Each case first proves its tie on an independent float32
restatement of the fill -- the two candidates have the same bits and beat every other -- and then asserts which one
msv_aln_oa takes.  (The arrays need not be posteriors of any model: the definition is a function of five arrays.)"""
import numpy as np
import pytest

import hmm_fasta_viterbi_amd as msv
from align_lib import path_key
from forward_lib import MM, MI, MD, IM, II, DM, DD

F = np.float32
NINF = F(-np.inf)
LENG = 4
NO_J = -np.inf  # tr_E_J that keeps J out of reach


def blank(Le):
    M = LENG + 1
    return {"pm": np.zeros((Le, M), F), "pi": np.zeros((Le, M), F), "pn": np.zeros(Le, F), "pj": np.zeros(Le, F),
            "pc": np.zeros(Le, F)}


def fill(p, tsc, consts):
    """The recurrence of msv.h restated: every value of every row, float32."""
    tBM, tEC, tEJ = consts
    Le, M = p["pm"].shape
    K = M - 1
    via = lambda x, t: x if np.isfinite(t) else NINF
    Mv, Iv, Dv = (np.full((Le + 1, M + 1), NINF, F) for _ in range(3))
    N, J, C, B, E = (np.full(Le + 1, NINF, F) for _ in range(5))
    N[0], B[0] = F(0), F(0)
    for i in range(1, Le + 1):
        for k in range(1, K + 1):
            Mv[i, k] = max(m_candidates(Mv, Iv, Dv, B, tsc, tBM, i, k)) + p["pm"][i - 1, k]
            if k < K:
                Iv[i, k] = max(via(Mv[i - 1, k], tsc[k, MI]), via(Iv[i - 1, k], tsc[k, II])) + p["pi"][i - 1, k]
        for k in range(2, K + 1):
            Dv[i, k] = max(via(Mv[i, k - 1], tsc[k - 1, MD]), via(Dv[i, k - 1], tsc[k - 1, DD]))
        E[i] = Mv[i, 1:K + 1].max()
        N[i] = N[i - 1] + p["pn"][i - 1]
        J[i] = max(J[i - 1] + p["pj"][i - 1], via(E[i], tEJ))
        C[i] = max(C[i - 1] + p["pc"][i - 1], via(E[i], tEC))
        B[i] = max(N[i], J[i])
    return {"M": Mv, "I": Iv, "D": Dv, "N": N, "J": J, "C": C, "B": B, "E": E}


def m_candidates(Mv, Iv, Dv, B, tsc, tBM, i, k):
    via = lambda x, t: x if np.isfinite(t) else NINF
    if k == 1:
        return [NINF, NINF, NINF, via(B[i - 1], tBM)]
    return [via(Mv[i - 1, k - 1], tsc[k - 1, MM]), via(Iv[i - 1, k - 1], tsc[k - 1, IM]),
            via(Dv[i - 1, k - 1], tsc[k - 1, DM]), via(B[i - 1], tBM)]


def candidates(v, p, tsc, consts, cell):
    """The candidates of a cell in msv.h's tie-break order."""
    kind, i, k = cell
    if kind == "M":
        return m_candidates(v["M"], v["I"], v["D"], v["B"], tsc, consts[0], i, k)
    if kind == "I":
        return [v["M"][i - 1, k], v["I"][i - 1, k]]
    if kind == "D":
        return [v["M"][i, k - 1], v["D"][i, k - 1]]
    if kind == "C":
        return [v["C"][i - 1] + p["pc"][i - 1], v["E"][i]]
    if kind == "J":
        return [v["J"][i - 1] + p["pj"][i - 1], v["E"][i]]
    if kind == "B":
        return [v["N"][i], v["J"][i]]
    raise KeyError(kind)


def dom(i_from, i_to, k_from, k_to, ops):
    out, i, k = [], i_from - 1, k_from - 1
    for op in ops:
        if op == "M":
            i, k = i + 1, k + 1
        elif op == "I":
            i += 1
        else:
            k += 1
        out.append((op, k, i))
    assert (i, k) == (i_to, k_to)
    return tuple(out)


def case_m(first, second):
    """M(3,3) with candidates `first` and `second` (of M, I, D, B) tied above the other two."""
    p = blank(3)
    p["pm"][2, 3] = 8
    if (first, second) == ("M", "I"):
        p["pm"][0, 1] = p["pm"][0, 2] = 1
        p["pm"][1, 2] = p["pi"][1, 2] = 0.5
        want = dom(1, 3, 1, 3, "MMM")
    elif (first, second) == ("M", "D"):
        p["pm"][0, 1] = p["pm"][1, 1] = 1
        want = dom(1, 3, 1, 3, "MMM")
    elif (first, second) == ("M", "B"):
        p["pn"][0], p["pn"][1] = 1, 0.5
        p["pm"][0, 1], p["pm"][1, 2] = 1, 0.5
        want = dom(1, 3, 1, 3, "MMM")
    elif (first, second) == ("I", "D"):
        p["pm"][1, 2] = -4
        p["pm"][0, 2], p["pi"][1, 2], p["pm"][1, 1] = 1, 0.5, 1.5
        want = dom(1, 3, 2, 3, "MIM")
    elif (first, second) == ("I", "B"):
        p["pn"][0], p["pn"][1] = 1, 0.5
        p["pm"][0, 2], p["pi"][1, 2] = 1, 0.5
        p["pm"][1, 2] = p["pm"][1, 1] = -4
        want = dom(1, 3, 2, 3, "MIM")
    else:  # D, B
        p["pn"][0], p["pn"][1] = 1, 0.5
        p["pm"][1, 1], p["pm"][1, 2] = 0.5, -4
        want = dom(2, 3, 1, 3, "MDM")
    order = "MIDB"
    return p, NO_J, ("M", 3, 3), order.index(first), order.index(second), (want,)


def case_i():
    p = blank(4)
    p["pm"][0, 1] = p["pm"][0, 2] = 1
    p["pm"][1, 2] = p["pi"][1, 2] = 0.5
    p["pi"][2, 2], p["pm"][3, 3] = 4, 8
    return p, NO_J, ("I", 3, 2), 0, 1, (dom(1, 4, 1, 3, "MMIM"),)


def case_d():
    p = blank(3)
    p["pm"][1, 1] = p["pm"][1, 2] = 2
    p["pm"][2, 4] = 8
    return p, NO_J, ("D", 2, 3), 0, 1, (dom(1, 3, 1, 4, "MMDM"),)


def case_e():
    p = blank(1)
    p["pm"][0, 2] = p["pm"][0, 4] = 3
    return p, NO_J, ("E", 1, 0), 2, 4, (dom(1, 1, 2, 2, "M"),)


def case_c():
    p = blank(2)
    p["pm"][0, 1], p["pc"][1], p["pm"][1, 2] = 2, 1, 1
    return p, NO_J, ("C", 2, 0), 0, 1, (dom(1, 1, 1, 1, "M"),)


def case_j():
    p = blank(3)
    p["pm"][0, 1], p["pj"][1], p["pm"][1, 2], p["pm"][2, 1] = 2, 1, 1, 8
    return p, -1.0, ("J", 2, 0), 0, 1, (dom(1, 1, 1, 1, "M"), dom(3, 3, 1, 1, "M"))


def case_b():
    p = blank(2)
    p["pn"][0], p["pm"][0, 1], p["pm"][1, 1] = 2, 2, 8
    return p, -1.0, ("B", 1, 0), 0, 1, (dom(2, 2, 1, 1, "M"),)


CASES = {
    "M takes M before I": lambda: case_m("M", "I"), "M takes M before D": lambda: case_m("M", "D"),
    "M takes M before B": lambda: case_m("M", "B"), "M takes I before D": lambda: case_m("I", "D"),
    "M takes I before B": lambda: case_m("I", "B"), "M takes D before B": lambda: case_m("D", "B"),
    "I takes M before I": case_i, "D takes M before D": case_d, "E takes the smallest k": case_e,
    "C takes the loop before E": case_c, "J takes the loop before E": case_j, "B takes N before J": case_b,
}


def test_there_are_twelve():
    assert len(CASES) == 12


@pytest.mark.parametrize("rule", sorted(CASES))
def test_tie_break(rule):
    p, tEJ, cell, first, second, want = CASES[rule]()
    tsc = np.full((LENG + 1, 7), F(-1.0))
    consts = (-1.0, -1.0, tEJ)
    v = fill(p, tsc, consts)
    bits = lambda x: np.asarray(x, F).view(np.uint32)
    if cell[0] == "E":  # the candidates are the row's M values, first and second the tied nodes
        row = v["M"][cell[1], 1:LENG + 1]
        assert bits(row[first - 1]) == bits(row[second - 1]) == bits(v["E"][cell[1]])
        assert all(row[k - 1] < row[first - 1] for k in range(1, LENG + 1) if k not in (first, second))
    else:
        cand = candidates(v, p, tsc, consts, cell)
        assert np.isfinite(cand[first]) and bits(cand[first]) == bits(cand[second]), (rule, cand)
        assert all(c < cand[first] for x, c in enumerate(cand) if x not in (first, second)), (rule, cand)
    post = (p["pm"], p["pi"], p["pn"], p["pj"], p["pc"])
    score, doms, ops, op_pp = msv.aln_oa(*post, tsc, consts)
    assert bits(score) == bits(v["C"][-1])
    assert path_key(doms, ops) == want, rule
    # the other choice scores the same, so only the order decides: nudging the second candidate's cell up by a
    # quarter must move the path (the case would prove nothing if the first candidate won regardless)
    if cell[0] == "M" and (first, second) == (0, 1):
        q = {k: a.copy() for k, a in p.items()}
        q["pi"][1, 2] += F(0.25)
        other = msv.aln_oa(q["pm"], q["pi"], q["pn"], q["pj"], q["pc"], tsc, consts)
        assert path_key(other[1], other[2]) != want
