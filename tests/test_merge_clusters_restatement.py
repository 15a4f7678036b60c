"""CPU: tests/merge_clusters_numpy.py against tests/golden/merge_clusters_reference.npz (scripts/make_merge_clusters_golden.py: the stage loop
with scipy's linkage, pandas' groupby median and the stage's cell order).  On every fixture the restatement's medoids and Z of every
iteration equal the file's bit for bit, and so do the step log, the counts and the final labels -- although the restatement orders the
cells of a pair by (group, cell) and the file by cell: the recorder rejects fixtures in which a rounding could decide.  Hand cases: the
median of 1, 2 and 3 values and of -0 / +0, the linkage of three collinear points, the tie rule, the label shift when leaf1 < max."""
import os

import numpy as np
import pytest

import merge_clusters_numpy as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "merge_clusters_reference.npz")
COUNTS = ("n_tests", "n_skipped", "n_merges", "n_iterations", "n_clusters_in", "n_clusters_out")


@pytest.fixture(scope="module")
def ref():
    return np.load(GOLDEN)


def check_against_file(ref, name, o, iterations=None):
    """o: the dict of merge_clusters (restatement or engine); iterations: [(medoids, Z)] or None"""
    tab, flat, off = M.steps_table(o["steps"])
    assert np.array_equal(tab, ref[name + ".steps"]), name
    assert np.array_equal(flat, ref[name + ".step_groups"]) and np.array_equal(off, ref[name + ".step_group_offsets"]), name
    assert [o[k] for k in COUNTS] == ref[name + ".counts"].tolist(), name
    assert np.array_equal(o["labels"], ref[name + ".labels"]), name
    if iterations is not None:
        assert len(iterations) == o["n_iterations"]
        for i, (medoids, Z) in enumerate(iterations):
            assert medoids.tobytes() == ref["%s.medoids.%d" % (name, i)].tobytes(), (name, i)
            assert Z.tobytes() == ref["%s.Z.%d" % (name, i)].tobytes(), (name, i)


@pytest.mark.parametrize("name", sorted(M.FIXTURES))
def test_restatement_equals_the_file(ref, name):
    x, pca, labels = M.fixture(name, int(ref[name + ".bump"]))
    trace = []
    o = M.merge_clusters(x, pca, labels, trace=trace)
    check_against_file(ref, name, o, [(t[1], t[2]) for t in trace if t[0] == "iteration"])
    min_q = np.array([t[1] for t in trace if t[0] == "test"])
    assert np.allclose(min_q, ref[name + ".min_q"], rtol=1e-9, atol=0)      # the cell order moves last bits of the sums only


def test_the_fixtures_do_what_they_are_for(ref):
    c = {n: dict(zip(COUNTS, ref[n + ".counts"].tolist())) for n in M.FIXTURES}
    assert (c["oversplit"]["n_clusters_in"], c["oversplit"]["n_clusters_out"]) == (6, 3)
    assert (c["distinct"]["n_clusters_out"], c["distinct"]["n_tests"], c["distinct"]["n_merges"]) == (4, 2, 0)
    assert (c["all_one"]["n_clusters_in"], c["all_one"]["n_clusters_out"]) == (4, 1)
    assert c["cached_pair"]["n_skipped"] == 1 and ref["cached_pair.steps"][-1].tolist() == [2, 0, 1, 1, -1, 0]
    assert np.all(ref["unused_barcodes.labels"][::3] == 0) and np.all(np.delete(ref["unused_barcodes.labels"], np.s_[::3]) > 0)
    _, _, lab = M.fixture("small_clusters", int(ref["small_clusters.bump"]))
    assert sorted(np.bincount(lab)[1:].tolist())[:2] == [1, 2]
    off, flat = ref["wide.step_group_offsets"], ref["wide.step_groups"]
    sizes = np.diff(off).reshape(-1, 2)
    assert c["wide"]["n_clusters_in"] == 17 and np.any((sizes.max(axis=1) >= 3) & (sizes.min(axis=1) == 2)) and len(flat) == off[-1]
    assert int(ref["n_rejected"]) >= 0


def test_median_hand_cases():
    pca = np.array([[5.0, -0.0], [1.0, 0.0], [2.0, 7.0], [4.0, 1.0], [9.0, 3.0], [3.0, 2.0]])
    med = M.cluster_medians(pca, np.array([0, 1, 1, 2, 2, 2]), 3)
    assert med.tolist() == [[5.0, 0.0], [1.5, 3.5], [4.0, 2.0]]
    assert M.cluster_medians(np.array([[-0.0], [0.0]]), np.array([0, 0]), 1)[0, 0] == 0.0


def test_linkage_hand_cases():
    Z = M.linkage_complete(np.array([[0.0], [1.0], [3.0]]))      # collinear: (0, 1) at 1, then {0, 1} with 2 at the LARGEST distance 3
    assert Z.tolist() == [[0.0, 1.0, 1.0, 2.0], [2.0, 3.0, 3.0, 3.0]]
    Z = M.linkage_complete(np.array([[0.0], [1.0], [2.0], [3.0]]))   # three distances of 1: the smallest (height, id0, id1) first
    assert Z.tolist() == [[0.0, 1.0, 1.0, 2.0], [2.0, 3.0, 1.0, 2.0], [4.0, 5.0, 3.0, 4.0]]
    assert M.linkage_complete(np.array([[0.0, 0.0], [3.0, 4.0]])).tolist() == [[0.0, 1.0, 5.0, 2.0]]


def test_label_shift_when_leaf1_is_not_the_largest():
    # three clusters: 0 and 1 are siblings without a difference, 2 is far away and different: 1 joins 0 and 2 becomes 1
    rs = np.random.RandomState(5)
    c = np.zeros((2, M.PCS))
    c[1, 0] = 50.0
    x, pca, truth = M._well(rs, [120, 80], c)
    labels = np.where(truth == 1, 3, 1 + (np.arange(len(truth)) % 2))
    o = M.merge_clusters(x, pca, labels)
    assert (o["n_clusters_in"], o["n_clusters_out"], o["n_merges"]) == (3, 2, 1)
    s = o["steps"]
    assert (s[0]["leaf0"], s[0]["leaf1"], s[0]["merged"]) == (0, 1, True) and (s[1]["leaf0"], s[1]["leaf1"], s[1]["groups0"], s[1]["groups1"]) == (0, 1, [0, 1], [2])
    assert np.array_equal(o["labels"], np.where(truth == 1, 2, 1))
