"""What a threshold costs in sensitivity, and what the later stages recover of the truth.

    python tools/emit_power.py --profile 100 --n 2000
    python tools/emit_power.py --profile all --n 2000 --out profiles       # profiles/emit_power_<profile>.jsonl

For a profile, N sequences are drawn from the model on the GPU (Emitter.emit) with their true domains and ops, and
search_pipeline runs on them twice: with the file's statistics and with calibrate()'s (the engines' own).  Recorded
per run: the share of the N sequences passing each of F1 (MSV), the bias filter, F2 (Viterbi) and F3 (Forward); over
the sequences that reach the domain stage, the share of the true match cells (i, k) that align_batch's
optimal-accuracy path recovers (over all cells, and the mean per true domain), and the share of true domains that a
decoded region (decode_batch) and a split item (split_regions) finds -- overlaps at least half of its residues --
with the mean absolute error of that region's two end points.  search_pipeline takes host batches, so the emitted
batch is downloaded once and uploaded by the pipeline; the chained device path is tests/test_gpu_emit.py's.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PROFILES = ("100", "1400", "2405")


def _cells(domains, ops):
    """{seq: set of (i, k)} of the 'M' ops of a Traces / Alignments-style (domains, ops) in parent coordinates."""
    out = {}
    for d in domains:
        i, k = int(d["i_from"]) - 1, int(d["k_from"]) - 1
        cells = out.setdefault(int(d["seq"]), set())
        for op in ops[int(d["ops_begin"]):int(d["ops_begin"]) + int(d["ops_len"])]:
            if op == 77:
                i, k = i + 1, k + 1
                cells.add((i, k))
            elif op == 73:
                i += 1
            else:
                k += 1
    return out


def _found(true_doms, spans):
    """Per true domain: the span (seq, i_from, i_to) that overlaps it most, if by at least half of its residues ->
    (share found, mean |start error|, mean |end error|)."""
    by_seq = {}
    for s, a, b in spans:
        by_seq.setdefault(int(s), []).append((int(a), int(b)))
    hit, e_from, e_to = 0, [], []
    for d in true_doms:
        a, b = int(d["i_from"]), int(d["i_to"])
        best, best_ov = None, 0
        for x, y in by_seq.get(int(d["seq"]), ()):
            ov = min(b, y) - max(a, x) + 1
            if ov > best_ov:
                best, best_ov = (x, y), ov
        if best is not None and 2 * best_ov >= b - a + 1:
            hit += 1
            e_from.append(abs(best[0] - a))
            e_to.append(abs(best[1] - b))
    n = max(len(true_doms), 1)
    return hit / n, float(np.mean(e_from)) if e_from else None, float(np.mean(e_to)) if e_to else None


def power(name, n, seed, length, F1, F2, F3):
    import hmm_fasta_viterbi_amd as msv
    profile = msv.Profile_HMM(os.path.join(ROOT, "data", "profile_HMMs", f"{name}.hmm"))
    engines = (msv.MSV_HMM(profile), msv.Viterbi_HMM(profile), msv.Forward_HMM(profile))
    dom, bias = msv.Domain_HMM(profile), msv.Bias_filter(profile)
    emitted = msv.Emitter(profile, length=length).emit(n, seed=seed, scores=False)
    truth = emitted.traces
    cal = msv.calibrate(profile, *engines)
    rows = []
    for label, stats in (("file", None), ("calibrated", cal)):
        r = msv.search_pipeline(*engines, codes=emitted.codes, offsets=emitted.offsets, F1=F1, F2=F2, F3=F3,
                                dom_engine=dom, align=True, bias_engine=bias, split=True, stats=stats)
        hits = set(int(s) for s in r["envelopes"].select)
        true_doms = truth.domains[np.isin(truth.domains["seq"], list(hits))]
        want = _cells(true_doms, truth.ops)
        aln = r["alignments"]
        got = _cells(aln.domains, aln.ops)
        n_true = sum(len(c) for c in want.values())
        n_both = sum(len(c & got.get(s, set())) for s, c in want.items())
        per_domain = []
        for d in true_doms:
            c = _cells([d], truth.ops)[int(d["seq"])]
            per_domain.append(len(c & got.get(int(d["seq"]), set())) / max(len(c), 1))
        reg = r["envelopes"].regions
        decoded = _found(true_doms, zip(reg["seq"], reg["i_from"], reg["i_to"]))
        it = r["split"]["items"]
        split = _found(true_doms, zip(it["seq"], it["i_from"], it["i_to"]))
        rows.append({
            "profile": f"{name}.hmm", "stats": label, "n": n, "seed": seed, "length": length,
            "F1": F1, "F2": F2, "F3": F3,
            "six": [float(x) for x in (cal.stats if stats is not None else cal.from_file)],
            "pass_F1": float(r["passed_msv"].mean()), "pass_bias": float(r["passed_bias"].mean()),
            "pass_F2": float(r["passed_vit"].mean()),
            "pass_F3": float((r["passed_vit"] & (r["fwd_pvalues"] <= F3)).mean()),
            "true_domains": int(len(truth.domains)), "true_domains_at_domain_stage": int(len(true_doms)),
            "match_cells_recovered": n_both / max(n_true, 1),
            "match_cells_recovered_per_domain_mean": float(np.mean(per_domain)) if per_domain else None,
            "domains_found_by_decode": decoded[0], "decode_start_error": decoded[1], "decode_end_error": decoded[2],
            "domains_found_by_split": split[0], "split_start_error": split[1], "split_end_error": split[2],
            "regions": int(len(reg)), "split_items": int(len(it)),
            "multidomain_regions": int(r["split"]["multidomain"].sum())})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--profile", default="all", choices=("all",) + PROFILES)
    ap.add_argument("--n", type=int, default=2000)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--length", type=int, default=400, help="the configured length Lc")
    ap.add_argument("--F1", type=float, default=0.02)
    ap.add_argument("--F2", type=float, default=1e-3)
    ap.add_argument("--F3", type=float, default=1e-5)
    ap.add_argument("--out", default="", help="directory for emit_power_<profile>.jsonl (default: print only)")
    a = ap.parse_args()
    for name in (PROFILES if a.profile == "all" else [a.profile]):
        rows = power(name, a.n, a.seed, a.length, a.F1, a.F2, a.F3)
        for row in rows:
            row["command"] = (f"python tools/emit_power.py --profile {name} --n {a.n} --seed {a.seed} "
                              f"--length {a.length} --F1 {a.F1} --F2 {a.F2} --F3 {a.F3}")
            print(json.dumps(row), flush=True)
        if a.out:
            os.makedirs(a.out, exist_ok=True)
            with open(os.path.join(a.out, f"emit_power_{name}.jsonl"), "w") as f:
                for row in rows:
                    f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
