"""Records the kernel plans every model length gets on this device into tests/golden/msv_plans.json.

    python tools/record_msv_plans.py [--out tests/golden/msv_plans.json]

The plans of a profile depend only on its model length, on tr_E_C == tr_E_J, on a forced variant and on the
device (csrc/msv_plan.cpp), so the record is taken per length: the 24 profiles of data/profile_HMMs, every
capacity C and C + 1 of the compiled MSV, cooperative and Viterbi families (AUTO_CAPACITIES of
tests/test_gpu_state_boundaries.py, on the seeded synthetic models those tests write), and three forced variants
(16 lanes, 64 lanes, split).  Per record: the whole describe() dictionary and variant_for(n) at n = 1, at each of
coop_max_n, latency_max_n and mid_max_n, at each of those plus one, and at 10**7.  The device's CU count goes
with them: tests/cpp/sanitize_host.cpp replays the choice on the CPU from this file, and
tests/test_gpu_configs.py compares a device's plans against it.  Run it on the commit whose plans are to be
kept, before changing the policy.
"""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FORCED = [("1400.hmm", "msv_g16_s88_w16_p2_d1"), ("2405.hmm", "msv_g64_s64_w12_p2_d1"),
          ("2405.hmm", "msv_g32_s76_a64_w16_p2_d1")]


def record(engine, source, forced=""):
    if forced:
        engine.set_variant(forced)
    d = engine.describe()
    points = {1, 10**7}
    for key in ("coop_max_n", "latency_max_n", "mid_max_n"):
        points |= {d[key], d[key] + 1}
    return {"source": source, "states": d["model_length"] - 1, "forced": forced, "describe": d,
            "variant_for": [[n, engine.variant_for(n)] for n in sorted(points)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "msv_plans.json"))
    args = ap.parse_args()
    import torch
    import hmm_fasta_viterbi_amd as msv
    from hmm_fasta_viterbi_amd.synthetic import write_hmm
    from test_gpu_state_boundaries import AUTO_CAPACITIES, MAX_STATES

    prof_dir = os.path.join(ROOT, "data", "profile_HMMs")
    records = []
    for name in sorted(os.listdir(prof_dir), key=lambda f: (len(f), f)):
        e = msv.MSV_HMM(msv.Profile_HMM(os.path.join(prof_dir, name)))
        records.append(record(e, name))
        e.close()
    with tempfile.TemporaryDirectory() as tmp:
        for leng in sorted({c + d for c in AUTO_CAPACITIES for d in (0, 1) if c + d <= MAX_STATES}):
            path = os.path.join(tmp, f"syn{leng}.hmm")
            write_hmm(path, leng, 9000 + leng)
            e = msv.MSV_HMM(msv.Profile_HMM(path))
            records.append(record(e, "synthetic"))
            e.close()
            os.remove(path)
    for name, forced in FORCED:
        e = msv.MSV_HMM(msv.Profile_HMM(os.path.join(prof_dir, name)))
        records.append(record(e, name, forced))
        e.close()
    props = torch.cuda.get_device_properties(0)
    out = {"device_name": props.name, "cus": props.multi_processor_count, "records": records}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write('{"device_name": %s, "cus": %d, "records": [\n' % (json.dumps(out["device_name"]), out["cus"]))
        f.write(",\n".join(json.dumps(r) for r in records))
        f.write("\n]}\n")
    print(f"{len(records)} records, {out['cus']} CUs -> {args.out}")


if __name__ == "__main__":
    main()
