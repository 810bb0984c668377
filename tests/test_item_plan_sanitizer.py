"""The chunked host calls' plan under AddressSanitizer + UBSan (csrc/Makefile `asan_items`): a stand-alone program
(tests/cpp/sanitize_item_plan.cpp) over the host-only sources, run as tests/test_sanitizers.py runs the others."""
import os
import subprocess

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hmm_fasta_viterbi_amd", "csrc")


def test_item_plan_sanitizer():
    p = subprocess.run(["make", "-s", "-C", CSRC, "asan_items"], capture_output=True, text=True, timeout=900)
    out = p.stdout + p.stderr
    assert p.returncode == 0, out[-4000:]
    assert "sanitize_item_plan passed" in out
    assert "ERROR: AddressSanitizer" not in out and "runtime error:" not in out
