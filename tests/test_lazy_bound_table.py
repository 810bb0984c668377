"""The lazy-E bound table (msv_lazy_bound_table: per lane and residue, the largest emission score of the
lane's states) against a numpy restatement, on the CPU."""
import numpy as np
import pytest

import hmm_fasta_viterbi_amd as msv
from hmm_fasta_viterbi_amd import _native
from oracle_lib import profile_path


def numpy_bound_table(es, G, S):
    K = es.shape[1] - 1  # states 1..K
    padded = np.full((20, G * S), -np.inf, np.float32)
    padded[:, :min(K, G * S)] = es[:, 1:1 + G * S]
    out = np.full((21, G), np.inf, np.float32)
    out[:20] = padded.reshape(20, G, S).max(axis=2)
    return out


# 1400.hmm on the benchmark's plan; 1100.hmm on its own plan, whose last lane holds 20 states and 52 padding
# slots; 900.hmm on a layout that leaves the last lane nothing but padding; a 4-lane layout
@pytest.mark.parametrize("prof,G,S", [("1400.hmm", 16, 88), ("1100.hmm", 16, 72), ("900.hmm", 16, 64),
                                      ("100.hmm", 4, 28)])
def test_bound_table_matches_numpy(prof, G, S):
    h = msv.Profile_HMM(profile_path(prof))
    es = np.ascontiguousarray(h.msv_scores()[0], np.float32)
    K = es.shape[1] - 1
    assert G * S >= K
    got = np.full((21, G), 7.0, np.float32)
    assert _native.lib().msv_lazy_bound_table(es.ctypes.data, es.shape[1], G, S, got.ctypes.data) == 0
    want = numpy_bound_table(es, G, S)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.all(np.isposinf(got[20]))  # the poison row never passes the bound
    real = -(-K // S)  # lanes that hold a state
    assert np.all(np.isfinite(got[:20, :real])) and np.all(np.isneginf(got[:20, real:]))
    if prof == "1100.hmm":
        assert K - (G - 1) * S == 20  # the last lane is mostly padding, and the padding is ignored
        assert np.array_equal(got[:20, G - 1], es[:, 1 + (G - 1) * S:].max(axis=1))
    if prof == "900.hmm":
        assert real == G - 1


def test_bound_table_rejects_bad_arguments():
    out = np.zeros(21 * 16, np.float32)
    es = np.zeros((20, 11), np.float32)
    L = _native.lib()
    assert L.msv_lazy_bound_table(None, 11, 16, 4, out.ctypes.data) == 1
    assert L.msv_lazy_bound_table(es.ctypes.data, 11, 16, 4, None) == 1
    assert L.msv_lazy_bound_table(es.ctypes.data, 1, 16, 4, out.ctypes.data) == 1
    assert L.msv_lazy_bound_table(es.ctypes.data, 11, 0, 4, out.ctypes.data) == 1
