"""Time the split stage on the regions of dom_tune.py's lists, against the alignment stage's four launch
kinds on the same regions in the same run.

    python tools/spl_tune.py --list 1400 --take 512
    python tools/spl_tune.py --list all --take 256 --out profiles        # profiles/spl_tune_<list>.jsonl

Method: the decode (Domain_HMM.decode_batch) runs once on the first `take` sequences of the list and its regions are
the items -- all of them, multi-domain or not, so both stages do the same work.  Then `rounds` alternating rounds of
one align call and one sample call (200 samples, HMMER's default) each; every call reports the device times of its
launch kinds from HIP events around the launches of each chunk (msv_aln_result_stats, msv_spl_result_stats; the
sampler's two passes together), and the medians over the rounds are reported.  The bytes are the stage's own count:
the recording kernel writes 12 bytes a cell (fM, fI, fD) of 64 S x Le (padding slots included, as the kernel moves
them).  No target is set: DESIGN 4.14 records the figures.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from fwd_tune import LISTS, survivor_like  # noqa: E402

SAMPLES = 200


def time_list(key, take, rounds):
    import hmm_fasta_viterbi_amd as msv
    prof, n, length = LISTS[key]
    h = msv.Profile_HMM(os.path.join(ROOT, "data", "profile_HMMs", prof))
    codes, offsets = survivor_like(msv, h, 7, n, length)
    take = min(take, n)
    offsets = offsets[:take + 1].copy()
    codes = codes[:int(offsets[-1])]
    dom = msv.Domain_HMM(h)
    env = dom.decode_batch(codes=codes, offsets=offsets)
    regions = env.regions
    items = np.zeros(len(regions), [("seq", "<u4"), ("i_from", "<u4"), ("i_to", "<u4")])
    for f in ("seq", "i_from", "i_to"):
        items[f] = regions[f]
    Le = items["i_to"].astype(np.int64) - items["i_from"] + 1
    multi = 0
    for q in range(len(env)):
        b, e, _ = env.posteriors(q)
        for g in env.regions_of(q):
            multi += int(msv.dom_is_multidomain(b, e, int(g["i_from"]), int(g["i_to"])))
    info = dom.split_describe()
    dom.align_batch(codes=codes, offsets=offsets, items=items)  # warm-up: code objects loaded
    dom.sample_batch(codes=codes, offsets=offsets, items=items, n_samples=SAMPLES)
    kinds = {"align_forward": [], "align_backward": [], "align_fill": [], "align_walk": [], "forward": [], "sample": []}
    for _ in range(rounds):  # alternating, so drift and neighbours hit both alike
        a = dom.align_batch(codes=codes, offsets=offsets, items=items)
        for k in ("forward", "backward", "fill", "walk"):
            kinds["align_" + k].append(a.stats[k + "_ms"])
        s = dom.sample_batch(codes=codes, offsets=offsets, items=items, n_samples=SAMPLES)
        kinds["forward"].append(s.stats["forward_ms"])
        kinds["sample"].append(s.stats["sample_ms"])
    med = {k: float(np.median(v)) for k, v in kinds.items()}
    align = med["align_forward"] + med["align_backward"] + med["align_fill"] + med["align_walk"]
    row = {"list": key, "profile": prof, "sequences": take, "decoded_residues": int(offsets[-1]),
           "items": int(len(items)), "multidomain_items": multi, "item_residues": int(Le.sum()),
           "variant": info["variant"], "states_per_lane": info["states_per_lane"], "samples": SAMPLES,
           "segments": int(len(s.segments)), "truncated": int(s.stats["truncated"]), "chunks": int(s.stats["chunks"]),
           "matrix_bytes": int(s.stats["matrix_bytes"]), "rounds": rounds,
           "ms_med": {k: round(v, 4) for k, v in med.items()},
           "ms_min": {k: round(float(np.min(v)), 4) for k, v in kinds.items()},
           "forward_gbytes_per_s": round(s.stats["matrix_bytes"] / max(med["forward"], 1e-9) / 1e6, 1),
           "split_over_align": round((med["forward"] + med["sample"]) / max(align, 1e-9), 3),
           "sample_over_align": round(med["sample"] / max(align, 1e-9), 3),
           "scratch_bytes": {k: info[k + "_scratch_bytes"] for k in ("forward", "sample")},
           "timing": "HIP events around each chunk's launches of a kind, summed per call; median over rounds"}
    dom.close()
    return [row]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--list", default="all", choices=["all"] + list(LISTS))
    ap.add_argument("--take", type=int, default=512, help="sequences of the list that are decoded for their regions")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="", help="directory for spl_tune_<list>.jsonl (default: print only)")
    a = ap.parse_args()
    for key in (LISTS if a.list == "all" else [a.list]):
        rows = time_list(key, a.take, a.rounds)
        for row in rows:
            print(json.dumps(row), flush=True)
        if a.out:
            os.makedirs(a.out, exist_ok=True)
            with open(os.path.join(a.out, f"spl_tune_{key}.jsonl"), "w") as f:
                for row in rows:
                    f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
