"""The split stage's host half under AddressSanitizer + UBSan (csrc/Makefile `asan_split`): a stand-alone program
(tests/cpp/sanitize_split.cpp) over the host-only sources, run as tests/test_align_sanitizer.py runs its own."""
import os
import subprocess

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hmm_fasta_viterbi_amd", "csrc")


def test_split_host_sanitizer():
    p = subprocess.run(["make", "-s", "-C", CSRC, "asan_split"], capture_output=True, text=True, timeout=900)
    out = p.stdout + p.stderr
    assert p.returncode == 0, out[-4000:]
    assert "sanitize_split passed" in out
    assert "ERROR: AddressSanitizer" not in out and "runtime error:" not in out
