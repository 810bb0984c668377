"""Time the emit stage launch by launch, against two references in the same run.

    python tools/emit_tune.py --profile 100 --n 100000
    python tools/emit_tune.py --profile all --n 100000 --out profiles      # profiles/emit_tune_<profile>.jsonl

Method: the batch is emitted once to size the device buffers (Emitter.emit_device), then `rounds` alternating rounds
of (a) one msv_emit_batch_device call into those buffers, whose three launches -- count, scan, place -- are timed by
the HIP events the call records around each (Emitter.last_times), and (b) one msv_cal_generate_device launch that
writes the same number of residues (n sequences of the batch's mean length): the upper reference, a generator with no
walk, timed by events around it.  Medians over the rounds.  The host reference, what the feature replaces, is
synthetic.gapped_homolog_batch for `host_n` sequences on the host clock, scaled to n (it is a Python loop, linear in
the sequences).  No target is set: DESIGN 4.16 records the figures.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PROFILES = ("100", "1400", "2405")


def time_profile(name, n, length, rounds, host_n):
    import torch

    import hmm_fasta_viterbi_amd as msv
    from hmm_fasta_viterbi_amd import _native
    from hmm_fasta_viterbi_amd.synthetic import gapped_homolog_batch
    profile = msv.Profile_HMM(os.path.join(ROOT, "data", "profile_HMMs", f"{name}.hmm"))
    e = msv.Emitter(profile, length=length)
    dev = torch.device("cuda:0")
    st = torch.cuda.Stream(dev)
    batch = e.emit_device(n, seed=42, stream=st.cuda_stream)  # sizes the buffers; also the warm-up
    tot = batch["totals"]
    truth = _native.EmitTruth(batch["domain_offsets"].data_ptr(), batch["domains"].data_ptr(), tot["domains"],
                              batch["ops"].data_ptr(), tot["ops"], batch["truncated"].data_ptr())
    L = max(1, round(tot["residues"] / n))
    d_null = torch.zeros(n * L + 16, dtype=torch.uint8, device=dev)
    d_null_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    bg = np.ascontiguousarray(msv.background_frequencies(), np.float32)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def null_once():
        ev0.record(st)
        msv.check(_native.lib().msv_cal_generate_device(0, bg.ctypes.data, 42, 0, 0, n, L, d_null.data_ptr(),
                                                        d_null_off.data_ptr(), st.cuda_stream), "cal_generate_device")
        ev1.record(st)
        st.synchronize()
        return ev0.elapsed_time(ev1)

    null_once()
    kinds = {"count": [], "scan": [], "place": [], "null_generate": []}
    for _ in range(rounds):  # alternating, so drift and neighbours hit both alike
        e.emit_into(n, batch["codes_ptr"], tot["residues"], batch["offsets_ptr"], seed=42, truth=truth,
                    stream=st.cuda_stream)
        t = e.last_times()
        for k in ("count", "scan", "place"):
            kinds[k].append(t[k + "_ms"])
        kinds["null_generate"].append(null_once())
    med = {k: float(np.median(v)) for k, v in kinds.items()}
    emit_ms = med["count"] + med["scan"] + med["place"]
    t0 = time.perf_counter()
    gapped_homolog_batch(profile.match_emissions, 42, host_n, max(1, L - 50), L + 50)
    host_s = time.perf_counter() - t0
    info = e.describe()
    row = {"profile": f"{name}.hmm", "n": n, "length": length, "residues": tot["residues"], "domains": tot["domains"],
           "ops": tot["ops"], "truncated": tot["truncated"], "null_length": L, "rounds": rounds,
           "ms_med": {k: round(v, 4) for k, v in med.items()},
           "ms_min": {k: round(float(np.min(v)), 4) for k, v in kinds.items()},
           "emit_ms": round(emit_ms, 4), "emit_residues_per_us": round(tot["residues"] / max(emit_ms, 1e-9) / 1e3, 2),
           "emit_over_null": round(emit_ms / max(med["null_generate"], 1e-9), 2),
           "host_gapped_homolog_batch": {"sequences": host_n, "seconds": round(host_s, 3),
                                         "scaled_to_n_seconds": round(host_s * n / host_n, 1)},
           "vgprs": {k: info[k + "_vgprs"] for k in ("count", "place", "scan")},
           "scratch_bytes": {k: info[k + "_scratch_bytes"] for k in ("count", "place", "scan")},
           "table_bytes": info["table_bytes"],
           "timing": "HIP events around each launch; median over alternating rounds; host reference on the host clock"}
    e.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--profile", default="all", choices=("all",) + PROFILES)
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--length", type=int, default=400, help="the configured length Lc")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--host-n", type=int, default=0, help="sequences of the host reference (0: n)")
    ap.add_argument("--out", default="", help="directory for emit_tune_<profile>.jsonl (default: print only)")
    a = ap.parse_args()
    for name in (PROFILES if a.profile == "all" else [a.profile]):
        row = time_profile(name, a.n, a.length, a.rounds, a.host_n or a.n)
        row["command"] = (f"python tools/emit_tune.py --profile {name} --n {a.n} --length {a.length} "
                          f"--rounds {a.rounds} --host-n {a.host_n or a.n}")
        print(json.dumps(row), flush=True)
        if a.out:
            os.makedirs(a.out, exist_ok=True)
            with open(os.path.join(a.out, f"emit_tune_{name}.jsonl"), "w") as f:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
