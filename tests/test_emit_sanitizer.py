"""The emit stage's host half under AddressSanitizer + UBSan (csrc/Makefile `asan_emit`): a stand-alone program
(tests/cpp/sanitize_emit.cpp) over the host-only sources, run as tests/test_split_sanitizer.py runs its own."""
import os
import subprocess

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hmm_fasta_viterbi_amd", "csrc")


def test_emit_host_sanitizer():
    p = subprocess.run(["make", "-s", "-C", CSRC, "asan_emit"], capture_output=True, text=True, timeout=900)
    out = p.stdout + p.stderr
    assert p.returncode == 0, out[-4000:]
    assert "sanitize_emit passed" in out
    assert "ERROR: AddressSanitizer" not in out and "runtime error:" not in out
