"""The split stage's clustering and region test (msv_spl_cluster, msv_dom_is_multidomain; msv.h "Split stage") on
hand-made inputs that reach every threshold from both sides."""
import numpy as np
import pytest

import hmm_fasta_viterbi_amd as msv
from hmm_fasta_viterbi_amd import _native


def segs(*rows):
    a = np.zeros(len(rows), _native.SEGMENT_DTYPE)
    for j, r in enumerate(rows):
        a[j] = r
    return a


def clusters(rows, n_samples, **kw):
    return msv.spl_cluster(segs(*rows), n_samples, **kw)


def counts(rows, n_samples=2, **kw):
    """Cluster sizes with every cluster kept (min_posterior 0)."""
    return sorted(int(c) for c in clusters(rows, n_samples, min_posterior=0.0, **kw)["count"])


def test_residue_overlap_of_exactly_four_fifths_links():
    # both 10 residues and 10 nodes long, on one diagonal band (difference 2 <= 4): overlap 8 of 10
    a, b = (1, 10, 1, 10), (3, 12, 1, 10)
    assert counts([a, b]) == [2]
    # one residue less: 7 of 10.  The diagonals differ by 3, still within 4: only the overlap decides
    assert counts([a, (4, 13, 1, 10)]) == [1, 1]


def test_the_shorter_segment_sets_the_overlap():
    # 5 residues and nodes wholly inside 20, on one diagonal: 5 of min(5, 20) is all of the shorter one
    assert counts([(1, 20, 1, 20), (16, 20, 16, 20)]) == [2]
    # 10 long, 7 of them inside the longer one: 7 of 10 is short of 4/5 although it is 7 of 20 residues either way
    assert counts([(1, 20, 1, 20), (14, 23, 14, 23)]) == [1, 1]
    assert counts([(1, 20, 1, 20), (13, 22, 13, 22)]) == [2]


def test_node_overlap_of_exactly_four_fifths_links():
    a = (1, 10, 1, 10)
    assert counts([a, (1, 10, 3, 12)]) == [2]      # nodes 3..10 of 10: 8
    assert counts([a, (1, 10, 4, 13)]) == [1, 1]   # 7


def test_diagonal_difference_four_links_five_does_not():
    a = (1, 40, 1, 40)
    assert counts([a, (5, 40, 1, 40)]) == [2]          # start diagonal 4 apart, overlap 36 of 36
    assert counts([a, (6, 40, 1, 40)]) == [1, 1]       # 5 apart
    assert counts([a, (1, 40, 1, 36)]) == [2]          # end diagonal 4 apart, node overlap 36 of 36
    assert counts([a, (1, 40, 1, 35)]) == [1, 1]       # 5 apart
    assert counts([a, (6, 40, 1, 40)], max_diagdiff=5) == [2]


def test_a_chain_is_one_cluster():
    a, b, c = (1, 40, 1, 40), (5, 44, 1, 40), (9, 48, 1, 40)
    assert counts([a, c]) == [1, 1]  # 8 apart
    assert counts([a, b, c]) == [3]
    assert counts([c, a, b]) == [3]


def test_a_quarter_of_the_samples_keeps_a_cluster():
    big = [(1, 30, 1, 30)] * 150
    for n, kept in ((50, True), (49, False)):
        env = clusters(big + [(101, 130, 1, 30)] * n, 200)
        assert len(env) == (2 if kept else 1), (n, env)
        assert env[0]["count"] == 150 and env[0]["prob"] == np.float32(0.75)
        if kept:
            assert env[1]["count"] == 50 and env[1]["prob"] == np.float32(0.25)


def test_an_end_point_seen_in_two_percent_is_taken():
    # a cluster of 100: i_from 10 once (1 % < 2 %), 11 twice (exactly 2 %), 12 for the rest; i_to mirrored
    rows = [(10, 50, 2, 40)] + [(11, 50, 2, 40)] * 2 + [(12, 50, 2, 40)] * 94 + [(12, 51, 2, 40)] * 2 + [(12, 52, 2, 40)]
    env = clusters(rows, 100)
    assert len(env) == 1 and env[0]["count"] == 100
    assert (env[0]["i_from"], env[0]["i_to"]) == (11, 51)
    # the nodes alike
    rows = [(12, 50, 1, 40)] + [(12, 50, 2, 40)] * 2 + [(12, 50, 3, 40)] * 94 + [(12, 50, 3, 41)] * 2 + [(12, 50, 3, 42)]
    env = clusters(rows, 100)
    assert (env[0]["k_from"], env[0]["k_to"]) == (2, 41)


def test_envelopes_come_sorted_by_i_from():
    rows = [(201, 230, 1, 30)] * 60 + [(1, 30, 1, 30)] * 70 + [(101, 130, 1, 30)] * 70
    env = clusters(rows, 200)
    assert list(env["i_from"]) == [1, 101, 201]
    assert list(env["count"]) == [70, 70, 60]


def test_no_surviving_cluster_yields_nothing():
    rows = [(1 + 40 * j, 30 + 40 * j, 1, 30) for j in range(5)] * 39  # five clusters of 39 < 50
    assert len(clusters(rows, 200)) == 0
    assert len(clusters([], 200)) == 0


def test_bad_segments_are_refused():
    with pytest.raises(msv.MSVError):
        clusters([(5, 4, 1, 2)], 10)


def _region(begin, end, i_from, i_to, rt3):
    return msv.dom_is_multidomain(np.array(begin, np.float32), np.array(end, np.float32), i_from, i_to, rt3)


def test_is_multidomain_at_rt3_from_both_sides():
    # sums of eighths are exact in float32.  Region 2..7 of 8 residues; values outside the region must not count
    begin = [9.0, 0.125, 0, 0, 0, 0.125, 0, 9.0]
    end = [9.0, 0, 0.125, 0, 0, 0, 0.125, 9.0]
    # Esum(z) for z = 2..7: 0, .125, .125, .125, .125, .25;  Bsum(z): .25, .125, .125, .125, .125, 0: the max of the
    # minima is 0.125
    assert _region(begin, end, 2, 7, 0.125)
    assert not _region(begin, end, 2, 7, float(np.nextafter(np.float32(0.125), np.float32(1))))
    assert _region(begin, end, 2, 7, float(np.nextafter(np.float32(0.125), np.float32(0))))
    # one domain: every end after every begin -> at no z are both sums positive ... except from z = the begin on
    assert not _region([0, 0.5, 0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0, 0.5, 0], 2, 7, 0.125)
    # the default is HMMER's 0.20
    assert msv.dom_is_multidomain(np.array(begin, np.float32) * 2, np.array(end, np.float32) * 2, 2, 7)
    assert not msv.dom_is_multidomain(np.array(begin, np.float32), np.array(end, np.float32), 2, 7)
    with pytest.raises(msv.MSVError):
        _region(begin, end, 0, 7, 0.2)
    with pytest.raises(msv.MSVError):
        _region(begin, end, 2, 9, 0.2)
