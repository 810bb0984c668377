"""Time the Forward stage's pick per S, and the Viterbi stage on the same list in the same run, on
survivor-like lists: sequences of about one length, device resident, one persistent launch each.

    python tools/fwd_tune.py --list 1400      1400.hmm x 7,000 sequences of length ~400
    python tools/fwd_tune.py --list 2405      2405.hmm x 11,000 sequences of length ~2,000
    python tools/fwd_tune.py --list 100       100.hmm x 260 sequences of length ~400
    python tools/fwd_tune.py --list all --out profiles

Method: both kernels warmed up on the list, then `rounds` alternating rounds of `reps` launches each, every launch
between two device events on its stream and synchronised before the events are read; the median launch is
reported with the minimum and the spread.  Rates count the kernels' own operations per cell (one cell = one model
state of one residue): GCUPS = cells / time; the VALU share is ops_per_cell x cells / time over the peak of
256 CUs x 128 lanes x 2.4 GHz.  Forward: 17 VALU operations per cell (M: 3 multiply/FMA + add + multiply; I: 2
(+1 with insert odds); D: 2 + the scan's fix-up FMA; E: 2 adds; plus the per-lane share of 6 scan steps and 6
reduction steps, ~3 at S = 22), FMA counted once.  Viterbi: 14, as tools/vit_tune.py.  The Forward scores are
checked against the float64 CPU Forward on a sample of the list before anything is timed.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FWD_OPS_PER_CELL = 17
VIT_OPS_PER_CELL = 14
VALU_PEAK_TOPS = 256 * 128 * 2.4e9 / 1e12
LISTS = {"1400": ("1400.hmm", 7000, 400), "2405": ("2405.hmm", 11000, 2000), "100": ("100.hmm", 260, 400)}


def survivor_like(msv, hmm, seed, n, length):
    """Homologs, one in eight of them gapped, of length within 10% of `length`, shuffled: what passes two filters."""
    from hmm_fasta_viterbi_amd.synthetic import concat_batches, gapped_homolog_batch, homolog_batch
    lo, hi = int(length * 0.9), int(length * 1.1)
    codes, offsets = concat_batches(homolog_batch(hmm.match_emissions, seed, n - n // 8, lo, hi),
                                    gapped_homolog_batch(hmm.match_emissions, seed + 1, n // 8, lo, hi))
    lens = np.diff(offsets.astype(np.int64))
    perm = np.random.Generator(np.random.PCG64(seed + 2)).permutation(n)
    parts = [codes[int(offsets[i]):int(offsets[i + 1])] for i in perm]
    off = np.zeros(n + 1, np.uint64)
    np.cumsum(lens[perm], out=off[1:])
    return np.concatenate(parts), off


def time_list(key, rounds, reps):
    import torch
    import hmm_fasta_viterbi_amd as msv
    prof, n, length = LISTS[key]
    h = msv.Profile_HMM(os.path.join(ROOT, "data", "profile_HMMs", prof))
    codes, offsets = survivor_like(msv, h, 7, n, length)
    leng = h.model_length - 1
    cells = int(offsets[-1]) * leng
    fwd, vit = msv.Forward_HMM(h), msv.Viterbi_HMM(h)
    dev = torch.device("cuda:0")
    r = torch.from_numpy(codes).to(dev)
    o = torch.from_numpy(offsets.view(np.int64)).to(dev)
    s = {k: torch.full((n,), float("nan"), dtype=torch.float32, device=dev) for k in ("fwd", "vit")}
    st = torch.cuda.Stream(dev)
    engines = {"fwd": fwd, "vit": vit}
    for e in engines.values():
        e.reserve_length(int(np.diff(offsets.astype(np.int64)).max()))

    def launch(k):
        engines[k].score_batch_device(r.data_ptr(), r.numel(), o.data_ptr(), n, s[k].data_ptr(),
                                      stream=st.cuda_stream)

    for k in engines:  # warm-up: code objects loaded, tables resident
        for _ in range(2):
            launch(k)
    torch.cuda.synchronize()
    fwd.check(st.cuda_stream)
    vit.check(st.cuda_stream)
    # results first: a sample of the list against the float64 CPU Forward, at msv.h's tolerance
    sample = np.arange(0, n, max(1, n // 32))[:32]
    got = s["fwd"].cpu().numpy()
    lens = np.diff(offsets.astype(np.int64))
    worst = 0.0
    for i in sample:
        ref = fwd.cpu_score_batch(codes=codes[int(offsets[i]):int(offsets[i + 1])],
                                  offsets=np.array([0, lens[i]], np.uint64))[0]
        tol = 16.0 * (lens[i] + leng) * 2.0 ** -24 + 4.0 * 2.0 ** -24 * abs(ref)
        assert abs(got[i] - ref) <= tol, (prof, int(i), float(got[i]), float(ref), tol)
        worst = max(worst, abs(got[i] - ref) / tol)
    times = {k: [] for k in engines}
    for _ in range(rounds):
        for k in engines:  # alternating, so drift and neighbours hit both alike
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                with torch.cuda.stream(st):
                    e0.record(st)
                    launch(k)
                    e1.record(st)
                st.synchronize()
                times[k].append(e0.elapsed_time(e1))
    rows = []
    for k, ops in (("fwd", FWD_OPS_PER_CELL), ("vit", VIT_OPS_PER_CELL)):
        t = np.array(times[k])
        ms = float(np.median(t))
        info = engines[k].describe()
        rows.append({"list": key, "profile": prof, "stage": k, "sequences": n, "length": length,
                     "residues": int(offsets[-1]), "cells": cells, "variant": info["variant"],
                     "states_per_lane": info["states_per_lane"], "blocks": info["blocks"],
                     "waves_per_block": info["waves_per_block"], "lds_bytes": info["lds_bytes"],
                     "scratch_bytes": info["scratch_bytes"], "launches": len(t), "ms_med": round(ms, 4),
                     "ms_min": round(float(t.min()), 4), "ms_p90": round(float(np.quantile(t, 0.9)), 4),
                     "gcups": round(cells / (ms * 1e-3) / 1e9, 1), "ops_per_cell": ops,
                     "valu_share": round(ops * cells / (ms * 1e-3) / 1e12 / VALU_PEAK_TOPS, 4),
                     "timing": "device events around one launch, synchronised; median of launches",
                     "fwd_worst_error_over_tolerance": round(worst, 4) if k == "fwd" else None})
    fwd.close()
    vit.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--list", default="all", choices=["all"] + list(LISTS))
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="", help="directory for fwd_tune_<list>.jsonl (default: print only)")
    a = ap.parse_args()
    for key in (LISTS if a.list == "all" else [a.list]):
        rows = time_list(key, a.rounds, a.reps)
        for row in rows:
            print(json.dumps(row), flush=True)
        if a.out:
            os.makedirs(a.out, exist_ok=True)
            with open(os.path.join(a.out, f"fwd_tune_{key}.jsonl"), "w") as f:
                for row in rows:
                    f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
