"""Time the bias filter's kernel against the MSV kernel on one resident batch, in one process.

    python tools/bias_filter_bench.py [--out profiles/bias_filter_cfg3.json]

The batch is bench.py's cfg3: 1400.hmm x 100,000 seeded sequences of 300 .. 500 residues, device resident.  The bias
kernel runs over EVERY sequence (in the cascade it only sees the MSV survivors), the MSV kernel over the same batch in
its longest-first order.  Method: both warmed up, then `launches` alternating launches each, every launch between two
device events on its stream and synchronised before the events are read; the median is reported with the minimum and
the 90th percentile.  A record, not a gate.  The bias of a sample is checked against the float64 definition at msv.h's
tolerance before anything is timed.
"""
import argparse
import datetime
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    import hmm_fasta_viterbi_amd as msv
    from hmm_fasta_viterbi_amd.synthetic import random_batch

    h = msv.Profile_HMM(os.path.join(ROOT, "data", "profile_HMMs", "1400.hmm"))
    codes, offsets = random_batch(2, 100_000, 300, 500)  # bench.py CONFIGS["cfg3"]
    n = len(offsets) - 1
    eng = {"bias": msv.Bias_filter(h), "msv": msv.MSV_HMM(h)}
    eng["msv"].reserve_length(500)
    dev = torch.device("cuda:0")
    r = torch.from_numpy(codes).to(dev)
    o = torch.from_numpy(offsets.view(np.int64)).to(dev)
    out = {k: torch.full((n,), float("nan"), dtype=torch.float32, device=dev) for k in eng}
    order = torch.zeros(n, dtype=torch.int32, device=dev)
    st = torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    eng["msv"].order_longest_first(o.data_ptr(), n, order.data_ptr(), st.cuda_stream)

    def launch(k):
        if k == "bias":
            eng[k].score_batch_device(r.data_ptr(), r.numel(), o.data_ptr(), n, out[k].data_ptr(),
                                      stream=st.cuda_stream)
        else:
            eng[k].score_batch_device(r.data_ptr(), r.numel(), o.data_ptr(), n, out[k].data_ptr(), order.data_ptr(),
                                      st.cuda_stream)

    for k in eng:  # warm-up: code objects loaded, tables resident
        for _ in range(3):
            launch(k)
    st.synchronize()
    eng["bias"].check(st.cuda_stream)
    eng["msv"].check(st.cuda_stream)
    got = out["bias"].cpu().numpy()
    sample = np.arange(0, n, n // 64)[:64]
    sub = [codes[int(offsets[i]):int(offsets[i + 1])] for i in sample]
    so = np.concatenate([[0], np.cumsum([len(x) for x in sub])]).astype(np.uint64)
    ref = eng["bias"].cpu_score(codes=np.concatenate(sub), offsets=so)
    ratio = np.abs(got[sample] - ref) / msv.Bias_filter.tolerance(np.diff(so), ref)
    assert np.all(ratio <= 1.0), ratio.max()
    times = {k: [] for k in eng}
    for _ in range(a.launches):
        for k in eng:  # alternating, so drift and neighbours hit both alike
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(st):
                e0.record(st)
                launch(k)
                e1.record(st)
            st.synchronize()
            times[k].append(e0.elapsed_time(e1))
    row = {"config": "cfg3", "profile": "1400.hmm", "sequences": n, "residues": int(offsets[-1]),
           "date": datetime.date.today().isoformat(), "launches": a.launches,
           "timing": "device events around one launch, synchronised, both kernels alternating; median of launches",
           "bias_variant": eng["bias"].describe()["variant"], "bias_blocks": eng["bias"].describe()["blocks"],
           "bias_vgprs": eng["bias"].describe()["vgprs"], "msv_variant": eng["msv"].variant_for(n),
           "bias_sample_worst_error_over_tolerance": round(float(ratio.max()), 4)}
    for k in eng:
        t = np.array(times[k])
        row[f"{k}_ms_med"] = round(float(np.median(t)), 4)
        row[f"{k}_ms_min"] = round(float(t.min()), 4)
        row[f"{k}_ms_p90"] = round(float(np.quantile(t, 0.9)), 4)
    row["bias_over_msv"] = round(row["bias_ms_med"] / row["msv_ms_med"], 4)
    row["bias_residues_per_s"] = round(row["residues"] / (row["bias_ms_med"] * 1e-3), 0)
    print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(row, indent=1) + "\n")
    for e in eng.values():
        e.close()


if __name__ == "__main__":
    main()
