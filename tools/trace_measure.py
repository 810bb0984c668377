"""Measure the Viterbi trace beside the scoring kernel on a bench config's MSV survivors.

    python tools/trace_measure.py --config cfg3 --out profiles/trace_cfg3.json

Builds the config's rank-0 batch as bench.py does, takes the MSV filter's survivors (filter_pipeline), and traces
the first chunk of them at the default workspace: fill ms, walk ms and the back-pointer bytes written (the
call's own HIP events, msv_vit_traces_stats), beside the SCORING kernel's ms for the same sequences in the same
run (msv_vit_score_batch_device over the same select list, torch events).  Median of --repeat calls after one
warm-up; one JSON record.  No gate: a slow ratio is a recorded fact.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {  # bench.py's: profile, sequences, lmin, lmax, seed
    "cfg3": ("1400.hmm", 100_000, 300, 500, 2),
    "cfg5": ("2405.hmm", 100_000, 1500, 2500, 4),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg3", choices=sorted(CONFIGS))
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    import hmm_fasta_viterbi_amd as msv
    from hmm_fasta_viterbi_amd import _native
    from hmm_fasta_viterbi_amd.synthetic import random_batch

    prof, n, lmin, lmax, seed = CONFIGS[a.config]
    hmm = msv.Profile_HMM(os.path.join(ROOT, "data", "profile_HMMs", prof))
    eng, vit = msv.MSV_HMM(hmm), msv.Viterbi_HMM(hmm)
    codes, offsets = random_batch(seed * 1000, n, lmin, lmax)
    _, mask, vsc, _ = msv.filter_pipeline(eng, vit, codes=codes, offsets=offsets)
    passed = np.flatnonzero(mask).astype(np.uint32)
    info = vit.trace_describe()
    L = _native.lib()
    plan = [name for name, _ in vit.trace_plans()].index(info["plan"])
    sizes = np.array([L.msv_vit_trace_sequence_bytes(plan, int(offsets[s + 1] - offsets[s])) for s in passed],
                     np.uint64)
    cuts = np.zeros(len(sizes) + 1, np.uint64)
    chunks = C.c_uint64()
    assert L.msv_vit_trace_chunk_cuts(sizes.ctypes.data, len(sizes), info["default_workspace_bytes"],
                                      cuts.ctypes.data, C.byref(chunks)) == 0
    first = passed[:int(cuts[1])] if chunks.value else passed[:0]

    fill, walk = [], []
    for it in range(a.repeat + 1):
        t = vit.trace_batch(codes=codes, offsets=offsets, select=first)
        if it:
            fill.append(t.stats["fill_ms"])
            walk.append(t.stats["walk_ms"])
    assert t.stats["chunks"] == 1
    assert np.array_equal(t.scores.view(np.uint32), vsc[first].view(np.uint32))

    # the scoring kernel on the same sequences, device-resident, timed with events on one stream
    dev = torch.device("cuda", 0)
    d_res = torch.from_numpy(codes).to(dev)
    d_off = torch.from_numpy(offsets.view(np.int64)).to(dev)
    d_sel = torch.from_numpy(first.view(np.int32)).to(dev)
    d_cnt = torch.tensor([len(first)], dtype=torch.int32, device=dev)
    d_sc = torch.zeros(n, dtype=torch.float32, device=dev)
    st = torch.cuda.Stream(dev)
    score = []
    torch.cuda.synchronize()
    for it in range(a.repeat + 3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(st):
            e0.record(st)
            vit.score_batch_device(d_res.data_ptr(), codes.size, d_off.data_ptr(), n, d_sc.data_ptr(),
                                   d_sel.data_ptr(), d_cnt.data_ptr(), st.cuda_stream)
            e1.record(st)
        st.synchronize()
        if it >= 3:
            score.append(e0.elapsed_time(e1))
    vit.check(st.cuda_stream)
    assert np.array_equal(d_sc.cpu().numpy()[first].view(np.uint32), t.scores.view(np.uint32))

    med = statistics.median
    rec = {
        "what": "Viterbi trace beside the scoring kernel, same sequences, same run (tools/trace_measure.py)",
        "config": a.config, "profile": prof, "sequences": n, "survivors": int(len(passed)),
        "chunks_at_default_workspace": int(chunks.value), "traced_first_chunk": int(len(first)),
        "traced_residues": int(sum(int(offsets[s + 1] - offsets[s]) for s in first)),
        "trace_plan": info["plan"], "scoring_variant": vit.describe()["variant"],
        "workspace_bytes": int(info["default_workspace_bytes"]), "pointer_bytes": int(t.stats["pointer_bytes"]),
        "domains": int(len(t.domains)), "ops": int(len(t.ops)),
        "fill_ms": med(fill), "walk_ms": med(walk), "score_ms": med(score),
        "fill_over_score": med(fill) / med(score), "trace_over_score": (med(fill) + med(walk)) / med(score),
        "fill_ms_all": fill, "walk_ms_all": walk, "score_ms_all": score, "repeat": a.repeat,
    }
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
