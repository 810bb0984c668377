"""Time the alignment stage on the regions of dom_tune.py's lists, against the decode's two launches in
the same run.

    python tools/aln_tune.py --list 1400 --take 512
    python tools/aln_tune.py --list all --take 256 --out profiles        # profiles/aln_null2_tune_<list>.jsonl
    python tools/aln_tune.py --list all --take 256 --ab profiles/aln_null2_ab_finish_loads.jsonl --label "..."

Method: the decode (Domain_HMM.decode_batch) runs once on the first `take` sequences of the list and its regions are
the items.  Then `rounds` alternating rounds of one decode call and one align call each; every call reports the
device times of its launch kinds from HIP events around the launches of each chunk (msv_dom_result_stats,
msv_aln_result_stats), and the medians over the rounds are reported.  The bytes are the stage's own count: the
recording kernel writes 8 bytes a cell (fM, fI), Backward reads and rewrites them, the fill reads them: 32 bytes a
cell of 64 S x Le (padding slots included, as the kernels move them).  No target is set: DESIGN 4.11 records the
figures beside the estimate.  The align calls run with the null2 option: its two launches have an event
pair of their own behind the count walk, so the four other kinds are timed as before; they read the matrix once, 8
bytes a cell.
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
    info = dom.align_describe()
    S = info["states_per_lane"]
    dom.align_batch(codes=codes, offsets=offsets, items=items, null2=True)  # warm-up: code objects loaded
    kinds = {"decode_forward": [], "decode_backward": [], "forward": [], "backward": [], "fill": [], "walk": [],
             "null2": [], "null2_partial": []}
    chunks = 0
    for _ in range(rounds):  # alternating, so drift and neighbours hit both alike
        e = dom.decode_batch(codes=codes, offsets=offsets)
        kinds["decode_forward"].append(e.stats["forward_ms"])
        kinds["decode_backward"].append(e.stats["backward_ms"])
        a = dom.align_batch(codes=codes, offsets=offsets, items=items, null2=True)
        for k in ("forward", "backward", "fill", "walk", "null2", "null2_partial"):
            kinds[k].append(a.stats[k + "_ms"])
        slab_bytes = a.stats["null2_slab_bytes"]
        chunks = a.stats["chunks"]
        matrix_bytes = a.stats["matrix_bytes"]
    med = {k: float(np.median(v)) for k, v in kinds.items()}
    moved = {"forward": matrix_bytes, "backward": 2 * matrix_bytes, "fill": matrix_bytes, "null2": matrix_bytes}
    row = {"list": key, "profile": prof, "sequences": take, "decoded_residues": int(offsets[-1]),
           "items": int(len(items)), "item_residues": int(Le.sum()), "variant": info["variant"],
           "states_per_lane": S, "chunks": int(chunks), "matrix_bytes": int(matrix_bytes), "rounds": rounds,
           "ms_med": {k: round(v, 4) for k, v in med.items()},
           "ms_min": {k: round(float(np.min(v)), 4) for k, v in kinds.items()},
           "gbytes_per_s": {k: round(moved[k] / (med[k] * 1e-3) / 1e9, 1) for k in moved if med[k] > 0},
           "align_over_decode": round((med["forward"] + med["backward"] + med["fill"] + med["walk"]) /
                                      max(med["decode_forward"] + med["decode_backward"], 1e-9), 3),
           "null2_row_block": info["null2_row_block"], "null2_slab_bytes": int(slab_bytes),
           "null2_over_fill": round(med["null2"] / max(med["fill"], 1e-9), 3),
           "null2_over_backward": round(med["null2"] / max(med["backward"], 1e-9), 3),
           "scratch_bytes": {k: info[k + "_scratch_bytes"]
                             for k in ("forward", "backward", "fill", "walk", "null2_partial", "null2_finish")},
           "timing": "HIP events around each chunk's launches of a kind, summed per call; median over rounds"}
    dom.close()
    return [row]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--list", default="all", choices=["all"] + list(LISTS))
    ap.add_argument("--take", type=int, default=512, help="sequences of the list that are decoded for their regions")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="", help="directory for <prefix>_<list>.jsonl (default: print only)")
    ap.add_argument("--prefix", default="aln_null2_tune",
                    help="file name prefix under --out (DESIGN 4.11's rows, taken before the null2 launches existed, are "
                         "profiles/aln_tune_<list>.jsonl and are not this tool's to overwrite)")
    ap.add_argument("--label", default="", help="with --ab: the `build` this run is recorded under")
    ap.add_argument("--ab", default="", help="append one trimmed row per list (build, list, variant, chunks, ms_med, "
                                             "rounds) to this file: an A/B of two builds is two runs with two labels")
    a = ap.parse_args()
    for key in (LISTS if a.list == "all" else [a.list]):
        rows = time_list(key, a.take, a.rounds)
        for row in rows:
            print(json.dumps(row), flush=True)
        if a.out:
            os.makedirs(a.out, exist_ok=True)
            with open(os.path.join(a.out, f"{a.prefix}_{key}.jsonl"), "w") as f:
                for row in rows:
                    f.write(json.dumps(row) + "\n")
        if a.ab:
            with open(a.ab, "a") as f:
                for row in rows:
                    f.write(json.dumps({"build": a.label, **{k: row[k] for k in ("list", "variant", "chunks", "ms_med",
                                                                                "rounds")}}) + "\n")


if __name__ == "__main__":
    main()
