"""The lazy-E rule of the long whole-row MSV kernels (msv_kernel_body.inc, LAZY), simulated in
float32 on the CPU with the kernel's exact rule: how many rows of a wave skip their E maximum.

Each lane of a G-lane group bounds its own states' M by U_t = emax_lane[r_t] + max3(U_{t-1}, M_left(t-1), Bt),
where M_left is the exact M of the left lane's last state that the row already shifts in.  Rounding is monotone,
so U_t >= the lane's exact E_t (asserted).  A wave of 64 / G sequences runs a LEAN row (no E maximum) only if no
lane of any of them has fl(U_t + tEJ) > fl(Jg + loop), Jg the group's J decayed by the same `+ loop` as the lane
partials; a full row resets U to the lane's exact maximum and re-reads Jg from the lane partials when some lane's
E + tEJ beats it.  The simulation keeps the kernel's per-lane J partials (a lean row only decays them) and checks
at every row that their group maximum is the reference's J, bit for bit.

Usage: python tools/lazy_e_bound_lanes.py [profile] [G] [--json OUT]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import hmm_fasta_viterbi_amd as msv
from hmm_fasta_viterbi_amd.synthetic import random_batch

F = np.float32
args = [a for a in sys.argv[1:] if not a.startswith("--")]
out_json = sys.argv[sys.argv.index("--json") + 1] if "--json" in sys.argv else None
if out_json:
    args.remove(out_json)
prof = args[0] if len(args) > 0 else '1400.hmm'
G = int(args[1]) if len(args) > 1 else 16
PER_WAVE = 64 // G
h = msv.Profile_HMM(os.path.join(ROOT, 'data', 'profile_HMMs', prof))
es, tBM, tEC, tEJ = h.msv_scores()          # es [20, Mcols]
Mcols = es.shape[1]; K = Mcols - 1            # states 1..K
S = -(-K // G)
S += -S % 4                                   # the kernels' lanes hold whole float4 chunks
E20 = np.full((20, G * S), -np.inf, F); E20[:, :K] = es[:, 1:]
emax = E20.reshape(20, G, S).max(axis=2)      # [20, G]: msv_lazy_bound_table's rows 0..19
SEED, NSEQ, LMIN, LMAX = 2, PER_WAVE * 400, 300, 500   # cfg3's lengths
codes, offs = random_batch(SEED, NSEQ, LMIN, LMAX)
nseq = len(offs) - 1
waves = nseq // PER_WAVE
rows_total = lean_rows = record_rows = seq_rows = seq_rows_passing = 0
for w in range(waves):
    seqs = [codes[offs[PER_WAVE*w+g]:offs[PER_WAVE*w+g+1]] for g in range(PER_WAVE)]
    Lmax = max(len(s) for s in seqs)
    st = []
    for s in seqs:
        L = len(s); loop, move = (F(x) for x in msv.sequence_transitions(L))
        st.append(dict(M=np.full(G*S, -np.inf, F), J=F(-np.inf), N=F(0), B=move, loop=loop, move=move,
                       U=np.full(G, -np.inf, F), Jl=np.full(G, -np.inf, F), Jg=F(-np.inf), s=s, L=L))
    for i in range(Lmax):
        full = False
        for d in st:
            if i >= d['L']: continue
            r = d['s'][i]
            Bt = F(d['B'] + F(tBM))
            prevM = d['M']
            sh = np.concatenate([[F(-np.inf)], prevM[:-1]]).astype(F)
            M = (E20[r] + np.maximum(sh, Bt)).astype(F)
            lastprev = prevM.reshape(G, S)[:, -1]
            left = np.concatenate([[F(-np.inf)], lastprev[:-1]]).astype(F)
            U = (emax[r] + np.maximum(np.maximum(d['U'], left), Bt)).astype(F)
            Elane = M.reshape(G, S).max(axis=1)
            assert np.all(U >= Elane)
            thr = F(d['Jg'] + d['loop'])
            d['need'] = bool(np.any((U + F(tEJ)).astype(F) > thr))
            d['Mnew'], d['Unew'], d['Elane'], d['thr'] = M, U, Elane, thr
            full |= d['need']
            seq_rows += 1; seq_rows_passing += not d['need']
        rows_total += 1; lean_rows += not full
        for d in st:
            if i >= d['L']: continue
            d['M'] = d['Mnew']
            # the reference's J
            E = d['Elane'].max()
            d['J'] = max(F(d['J'] + d['loop']), F(E + F(tEJ)))
            # the kernel's lane partials, bound and Jg
            d['Jg'] = d['thr']
            decayed = (d['Jl'] + d['loop']).astype(F)
            if full:
                EJ = (d['Elane'] + F(tEJ)).astype(F)
                d['Jl'] = np.maximum(decayed, EJ)
                d['U'] = d['Elane']
                if np.any(EJ > d['Jg']):
                    d['Jg'] = d['Jl'].max(); record_rows += 1
            else:
                d['Jl'] = decayed
                d['U'] = d['Unew']
            assert d['Jl'].max().view(np.uint32) == F(d['J']).view(np.uint32) and d['Jg'] <= d['J']
            d['N'] = F(d['N'] + d['loop'])
            d['B'] = F(max(d['N'], d['J']) + d['move'])
result = {
    "tool": "tools/lazy_e_bound_lanes.py", "profile": prof, "G": G, "S": S, "sequences_per_wave": PER_WAVE,
    "batch": {"seed": SEED, "sequences": nseq, "lmin": LMIN, "lmax": LMAX},
    "wave_rows": rows_total, "lean_wave_rows": int(lean_rows), "lean_fraction": round(lean_rows / rows_total, 4),
    "sequence_rows": seq_rows, "sequence_rows_passing_alone": int(seq_rows_passing),
    "sequence_pass_fraction": round(seq_rows_passing / seq_rows, 4),
    "jg_refreshes_per_sequence_row": round(record_rows / seq_rows, 4),
    "group_j_bitwise_equal_at_every_row": True,
    "emax_mean": float(emax[np.isfinite(emax)].mean()), "tr_B_Mk": float(tBM),
}
print(json.dumps(result))
if out_json:
    with open(out_json, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
