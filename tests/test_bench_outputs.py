"""bench.py's plain run and --dump-outputs: the options exist (CPU), and on the GPU a plain run of the smallest
config times exactly --steps steps, carries none of the --full blocks, and writes the last timed step's scores --
the config's seeded rank-0 batch, bitwise the oracle's on a leading sample."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle_lib import ROOT, OracleProfile, bits

sys.path.insert(0, ROOT)
import bench  # noqa: E402

FULL_ONLY = ("end_to_end", "viterbi_stage", "cpu_baseline", "latency_ceiling", "scores_finite_and_consistent",
             "clock_twin_scores_bitwise_equal")


def test_plain_run_is_the_default(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "3"])
    a = bench.parse()
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 3, False, None)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "out"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "out"


@pytest.mark.gpu
def test_plain_run_dumps_the_timed_scores(tmp_path):
    from hmm_fasta_viterbi_amd.synthetic import random_batch
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--config", "cfg2", "--dump-outputs", str(tmp_path / "out")],
                       capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout
    d = lines[0]
    assert d["steps"] == 3 and d["warmup"] == 1 and d["full"] is False and d["scores_finite"] is True
    assert d["ms_per_step"] > 0 and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert abs(d["value"] - d["config"]["residues_all_ranks"] / (d["ms_per_step"] * 1e-3) / 1e6) <= 1e-3 * d["value"]
    assert all(d.get(k) is None for k in FULL_ONLY), [k for k in FULL_ONLY if d.get(k) is not None]
    assert d["roofline"]["clock_GHz"] is None
    assert os.listdir(tmp_path / "out") == ["scores.npy"]
    got = np.load(tmp_path / "out" / "scores.npy")
    prof, n, lmin, lmax, seed, _ = bench.CONFIGS["cfg2"]
    assert got.dtype == np.float32 and got.shape == (n,)
    codes, offsets = random_batch(seed * 1000, n, lmin, lmax)  # rank 0's batch
    m = 512
    want = OracleProfile(prof[:-4]).score_batch(codes, offsets[: m + 1])
    assert np.array_equal(bits(got[:m]), bits(want))
    assert np.all(np.isfinite(got))
