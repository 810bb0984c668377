"""The engines' own statistics beside the file's (msv.h "Calibration"): for each bundled profile the
default calibration on the GPU (calibrate(): 200 x 200, 200 x 200, 200 x 100, seed 42) and one run at N = 100,000
sequences per set; per profile the calibrated minus the file's MSV mu / Viterbi mu / Forward tau in bits and the wall
time of each run (the first default run of a profile also pays the first launches of its engines, so a second one is
timed too).  Nothing is gated: the numbers are written down.  It supersedes none of tools/vit_calibration.py,
tools/fwd_calibration.py and tools/pvalue_calibration.py, which measure the gap this stage closes.

    python tools/calibrate_profiles.py --out profiles/calibration_own_vs_file.jsonl
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(msv, h, engines, **kw):
    t = time.perf_counter()
    cal = msv.calibrate(h, *engines, **kw)
    return cal, time.perf_counter() - t


def minus_file(cal):
    d = cal.stats.astype(float) - cal.from_file.astype(float)
    return {"msv_mu": round(float(d[0]), 4), "viterbi_mu": round(float(d[2]), 4), "forward_tau": round(float(d[4]), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--big-n", type=int, default=100000)
    ap.add_argument("--profiles", default="", help="comma-separated profile names (default: all bundled)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import hmm_fasta_viterbi_amd as msv
    from oracle_lib import PROFILES, profile_path
    names = [p for p in a.profiles.split(",") if p] or list(PROFILES)
    out = open(a.out, "w") if a.out else None
    for prof in names:
        h = msv.Profile_HMM(profile_path(prof))
        engines = (msv.MSV_HMM(h), msv.Viterbi_HMM(h), msv.Forward_HMM(h))
        first, t_first = timed(msv, h, engines)
        again, t_again = timed(msv, h, engines)
        assert again.stats.tobytes() == first.stats.tobytes()
        d = {"profile": prof, "model_length": h.model_length - 1, "seed": 42, "lambda": first.lambda_,
             "file": [round(float(x), 5) for x in first.from_file],
             "default": {"stats": [round(float(x), 5) for x in first.stats], "minus_file_bits": minus_file(first),
                         "forward_gumbel": [round(first.report["gmu"], 4), round(first.report["glam"], 4)],
                         "newton_iterations": first.report["iterations"], "first_wall_s": round(t_first, 4),
                         "wall_s": round(t_again, 4)}}
        if a.big_n:
            big, t_big = timed(msv, h, engines, n=a.big_n)
            d["big"] = {"n": a.big_n, "stats": [round(float(x), 5) for x in big.stats],
                        "minus_file_bits": minus_file(big),
                        "forward_gumbel": [round(big.report["gmu"], 4), round(big.report["glam"], 4)],
                        "newton_iterations": big.report["iterations"], "chunks": big.report["chunks"],
                        "wall_s": round(t_big, 4)}
        for e in engines:
            e.close()
        line = json.dumps(d)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
    if out:
        out.close()


if __name__ == "__main__":
    main()
