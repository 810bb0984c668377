"""Time the domain stage's decode (the recording Forward launch + the Backward launch) against the
Forward launch on the same survivor-like lists in the same run: device resident, persistent launches.

    python tools/dom_tune.py --list 1400      1400.hmm x 7,000 sequences of length ~400
    python tools/dom_tune.py --list 2405      2405.hmm x 11,000 sequences of length ~2,000
    python tools/dom_tune.py --list 100       100.hmm x 260 sequences of length ~400
    python tools/dom_tune.py --list all --out profiles

Method (tools/fwd_tune.py's): both warmed up on the list, then `rounds` alternating rounds of `reps` timings each,
every timing between two device events on its stream and synchronised before the events are read; medians are
reported with the minimum and the 90th percentile.  One decode timing covers both of its launches.  The posteriors of
a sample of the list are checked against the float64 CPU decode at msv.h's tolerance before anything is timed.  No
speed target hangs on these figures; from the operation count (two passes plus the per-row record) the decode was
expected at 2-2.5x the Forward launch.
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


def time_list(key, rounds, reps):
    import torch
    import hmm_fasta_viterbi_amd as msv
    prof, n, length = LISTS[key]
    h = msv.Profile_HMM(os.path.join(ROOT, "data", "profile_HMMs", prof))
    codes, offsets = survivor_like(msv, h, 7, n, length)
    leng = h.model_length - 1
    total = int(offsets[-1])
    cells = total * leng
    fwd, dom = msv.Forward_HMM(h), msv.Domain_HMM(h)
    dev = torch.device("cuda:0")
    r = torch.from_numpy(codes).to(dev)
    o = torch.from_numpy(offsets.view(np.int64)).to(dev)
    f32 = lambda m: torch.full((m,), float("nan"), dtype=torch.float32, device=dev)
    s_fwd, d_fwd, d_bck = f32(n), f32(n), f32(n)
    begin, end, occ = f32(total), f32(total), f32(total)
    ws_bytes = dom.workspace_bytes(total, n)
    ws = torch.zeros(ws_bytes // 4, dtype=torch.int32, device=dev)
    st = torch.cuda.Stream(dev)
    longest = int(np.diff(offsets.astype(np.int64)).max())
    fwd.reserve_length(longest)
    dom.reserve_length(longest)

    def launch(k):
        if k == "fwd":
            fwd.score_batch_device(r.data_ptr(), r.numel(), o.data_ptr(), n, s_fwd.data_ptr(), stream=st.cuda_stream)
        else:
            dom.decode_batch_device(r.data_ptr(), r.numel(), o.data_ptr(), n, d_fwd.data_ptr(), d_bck.data_ptr(),
                                    begin.data_ptr(), end.data_ptr(), occ.data_ptr(), ws.data_ptr(), ws_bytes,
                                    stream=st.cuda_stream)

    for k in ("fwd", "dom"):  # warm-up: code objects loaded, tables resident
        for _ in range(2):
            launch(k)
    torch.cuda.synchronize()
    fwd.check(st.cuda_stream)
    dom.check(st.cuda_stream)
    # results first: the recording kernel has the Forward kernel's bits, and a sample of the list is within msv.h's
    # posterior tolerance of the float64 CPU decode
    assert np.array_equal(d_fwd.cpu().numpy().view(np.uint32), s_fwd.cpu().numpy().view(np.uint32))
    got = [x.cpu().numpy() for x in (begin, end, occ)]
    lens = np.diff(offsets.astype(np.int64))
    worst = 0.0
    for i in np.arange(0, n, max(1, n // 8))[:8]:
        lo, hi = int(offsets[i]), int(offsets[i + 1])
        ref = dom.decode_on_sequence(codes=codes[lo:hi])
        tol = 48.0 * (lens[i] + leng) * 2.0 ** -24 + 8.0 * 2.0 ** -24
        for g, want in zip(got, ref[2:]):
            err = float(np.abs(g[lo:hi] - want).max())
            assert err <= tol, (prof, int(i), err, tol)
            worst = max(worst, err / tol)
    times = {"fwd": [], "dom": []}
    for _ in range(rounds):
        for k in times:  # alternating, so drift and neighbours hit both alike
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                with torch.cuda.stream(st):
                    e0.record(st)
                    launch(k)
                    e1.record(st)
                st.synchronize()
                times[k].append(e0.elapsed_time(e1))
    med = {k: float(np.median(v)) for k, v in times.items()}
    rows = []
    for k, engine in (("fwd", fwd), ("dom", dom)):
        t = np.array(times[k])
        info = engine.describe()
        rows.append({"list": key, "profile": prof, "stage": k, "sequences": n, "length": length, "residues": total,
                     "cells": cells, "variant": info["variant"], "states_per_lane": info["states_per_lane"],
                     "blocks": info["blocks"], "backward_blocks": info.get("backward_blocks"),
                     "waves_per_block": info["waves_per_block"], "lds_bytes": info["lds_bytes"],
                     "scratch_bytes": info["scratch_bytes"], "timings": len(t), "ms_med": round(med[k], 4),
                     "ms_min": round(float(t.min()), 4), "ms_p90": round(float(np.quantile(t, 0.9)), 4),
                     "gcups": round(cells / (med[k] * 1e-3) / 1e9, 1),
                     "over_forward_launch": round(med[k] / med["fwd"], 3),
                     "timing": "device events around the stage's launches, synchronised; median of timings",
                     "posterior_worst_error_over_tolerance": round(worst, 5) if k == "dom" else None})
    fwd.close()
    dom.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--list", default="all", choices=["all"] + list(LISTS))
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="", help="directory for dom_tune_<list>.jsonl (default: print only)")
    a = ap.parse_args()
    for key in (LISTS if a.list == "all" else [a.list]):
        rows = time_list(key, a.rounds, a.reps)
        for row in rows:
            print(json.dumps(row), flush=True)
        if a.out:
            os.makedirs(a.out, exist_ok=True)
            with open(os.path.join(a.out, f"dom_tune_{key}.jsonl"), "w") as f:
                for row in rows:
                    f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
