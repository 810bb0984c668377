"""Forward tau calibration record: for each bundled profile, score HMMER's p7_Tau sample -- 10,000 iid
background sequences of length 100 -- with the library's float64 CPU Forward (msv_fwd_cpu_score_batch, no GPU) and
write d = (the empirical 0.96-quantile of the bit scores) - tau (STATS LOCAL FORWARD) to
profiles/fwd_calibration.jsonl.  tests/test_gpu_forward.py holds the kernel's d to the recorded band.

    python tools/fwd_calibration.py [--n 10000] [--length 100] [--seed 2025] [--out profiles/fwd_calibration.jsonl]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import hmm_fasta_viterbi_amd as msv  # noqa: E402
from hmm_fasta_viterbi_amd import _native  # noqa: E402
from hmm_fasta_viterbi_amd.synthetic import background_batch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000)
    ap.add_argument("--length", type=int, default=100)
    ap.add_argument("--seed", type=int, default=2025)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fwd_calibration.jsonl"))
    args = ap.parse_args()
    L = _native.lib()
    codes, offsets = background_batch(args.seed, args.n, args.length)
    p1 = args.length / (args.length + 1.0)
    nullsc = args.length * np.log(p1) + np.log(1.0 - p1)
    pdir = os.path.join(ROOT, "data", "profile_HMMs")
    rows = []
    for name in sorted(os.listdir(pdir), key=lambda f: int(f.split(".")[0])):
        hmm = msv.Profile_HMM(os.path.join(pdir, name))
        M = hmm.model_length
        msc, isc, tsc = np.zeros((20, M), np.float32), np.zeros((20, M), np.float32), np.zeros((M, 7), np.float32)
        b, c, j = C.c_float(), C.c_float(), C.c_float()
        msv.check(L.msv_hmm_viterbi_scores(hmm._h, msv.INSERTS_ZERO, msc.ctypes.data, isc.ctypes.data, tsc.ctypes.data,
                                           C.byref(b), C.byref(c), C.byref(j)))
        sc = np.zeros(args.n, np.float64)
        msv.check(L.msv_fwd_cpu_score_batch(msc.ctypes.data, None, tsc.ctypes.data, M, b.value, c.value, j.value,
                                            codes.ctypes.data, offsets.ctypes.data, args.n, sc.ctypes.data))
        bits = (sc - nullsc) / np.log(2.0)
        q = float(np.quantile(bits, 0.96))
        tau, lam = hmm.stats_local_forward_theta, hmm.stats_local_forward_lambda
        # the tail's slope beyond the quantile: the maximum-likelihood lambda of an exponential tail
        tail = bits[bits > q] - q
        # tau is the base of the exponential tail (P = 1 there), not the quantile: a perfectly calibrated profile has
        # exp(-lambda d) = 0.04, that is d = ln(25) / lambda; `excess_bits` is what remains
        expected = float(np.log(25.0) / lam)
        row = {"profile": name, "LENG": M - 1, "tau": tau, "lambda": lam, "q96_bits": round(q, 4),
               "d_bits": round(q - tau, 4), "d_calibrated_bits": round(expected, 4),
               "excess_bits": round(q - tau - expected, 4), "tail_lambda_fit": round(float(1.0 / tail.mean()), 4),
               "n": args.n, "length": args.length, "seed": args.seed, "engine": "msv_fwd_cpu_score_batch (float64)"}
        rows.append(row)
        print(json.dumps(row), flush=True)
    d = [r["d_bits"] for r in rows]
    x = [r["excess_bits"] for r in rows]
    rows.append({"summary": "d_bits over the profiles", "min": min(d), "max": max(d), "mean": round(float(np.mean(d)), 4),
                 "excess_min": min(x), "excess_max": max(x), "excess_mean": round(float(np.mean(x)), 4)})
    print(json.dumps(rows[-1]))
    with open(args.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
