"""The calibration stage's host half under AddressSanitizer + UBSan (csrc/Makefile `asan_calibrate`): a stand-alone
program (tests/cpp/sanitize_calibrate.cpp) over the host-only sources, run as tests/test_split_sanitizer.py runs its
own."""
import os
import subprocess

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hmm_fasta_viterbi_amd", "csrc")


def test_calibrate_host_sanitizer():
    p = subprocess.run(["make", "-s", "-C", CSRC, "asan_calibrate"], capture_output=True, text=True, timeout=900)
    out = p.stdout + p.stderr
    assert p.returncode == 0, out[-4000:]
    assert "sanitize_calibrate passed" in out
    assert "ERROR: AddressSanitizer" not in out and "runtime error:" not in out
