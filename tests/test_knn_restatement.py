"""CPU-side checks of the k-nearest-neighbour stage (no GPU): the numpy restatement (tests/knn_numpy.py) equals what scikit-learn 1.7.2's
BallTree recorded in tests/golden/knn_reference.npz -- indices and distances bit for bit on the tie-free fixtures, distances bit for
bit and indices in (d2, index) order on the tied ones -- and a live BallTree on mid_5000 where scikit-learn imports;
crgpu_graphclust_num_neighbors against hand values; louvain_labels and relabel_by_size against hand cases."""
import os

import numpy as np
import pytest

import knn_numpy as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "knn_reference.npz")
IN_GOLDEN = [n for n in R.FIXTURES if n not in R.NOT_IN_GOLDEN]


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module", autouse=True)
def built_library():
    from cellranger_amd import build

    build.build()


def test_golden_file_holds_every_fixture_but_the_large_one(golden):
    assert sorted(golden.files) == sorted(n + s for n in IN_GOLDEN for s in ("_rows", "_ind", "_dist"))
    for name in IN_GOLDEN:
        n, k = len(R.FIXTURES[name]["x"]), R.FIXTURES[name]["k"]
        rows = golden[name + "_rows"]
        assert rows[0] == 0 and rows[-1] == n - 1 and (np.diff(rows) > 0).all()
        assert golden[name + "_ind"].shape == (len(rows), k) == golden[name + "_dist"].shape
        assert golden[name + "_ind"].dtype == np.int32 and golden[name + "_dist"].dtype == np.float64


@pytest.mark.parametrize("name", IN_GOLDEN)
def test_restatement_equals_the_recorded_balltree(golden, name):
    f = R.FIXTURES[name]
    ind, dist, d2 = R.expected(name)
    rows = golden[name + "_rows"]
    assert np.array_equal(dist[rows], golden[name + "_dist"])          # every bit
    assert np.array_equal(np.sqrt(d2), dist)
    if not f["tied"]:
        assert np.array_equal(ind[rows], golden[name + "_ind"])
    else:
        x = R.used(name)
        for r in rows[:40]:
            assert R.is_pair_order(x, int(r), ind[r], f["k"]), r


def test_the_duplicate_quirk_and_the_tie_rule():
    ind, dist, _ = R.expected("duplicates")
    # 150 = 7, 41 = 40, 3 = 299: the higher row of a pair drops the lower one and keeps itself at distance 0; the lower drops itself
    for lo, hi in ((7, 150), (40, 41), (3, 299)):
        assert ind[hi, 0] == hi and dist[hi, 0] == 0.0 and lo not in ind[hi]
        assert ind[lo, 0] == hi and dist[lo, 0] == 0.0 and lo not in ind[lo]
    ind, dist, d2 = R.expected("lattice")
    same = d2[:, :-1] == d2[:, 1:]
    assert same.any() and (ind[:, :-1][same] < ind[:, 1:][same]).all()      # equal d2: the lower index first


def test_restatement_equals_a_live_balltree_on_mid_5000():
    neighbors = pytest.importorskip("sklearn.neighbors")
    x, k = R.used("mid_5000"), R.FIXTURES["mid_5000"]["k"]
    dist, ind = neighbors.BallTree(x, leaf_size=40).query(x, k + 1)
    r_ind, r_dist, _ = R.expected("mid_5000")
    assert np.array_equal(ind[:, 1:], r_ind) and np.array_equal(dist[:, 1:], r_dist)


def test_num_neighbors_against_hand_values():
    from cellranger_amd import engine as E

    # -230 + 120 log10(n): 2 -> -193.9 (the clamp to 1), 100 -> 10, 2000 -> 166.1, 10^4 -> 250, 10^5 -> 370, 10^6 -> 490
    for n, k in ((2, 1), (100, 10), (2000, 166), (10 ** 4, 250), (10 ** 5, 370), (10 ** 6, 490), (3000, 187)):
        assert E.graphclust_num_neighbors(n) == k == R.num_neighbors(n), n
    # a half: 0.5 + 1 * log10(100) = 2.5 -> 2 and 1.5 + 2 = 3.5 -> 4 (half to even), not 3 and 4
    assert E.graphclust_num_neighbors(100, 1, 0.5, 1.0) == 2 == R.num_neighbors(100, 1, 0.5, 1.0)
    assert E.graphclust_num_neighbors(100, 1, 1.5, 1.0) == 4 == R.num_neighbors(100, 1, 1.5, 1.0)
    assert E.graphclust_num_neighbors(10 ** 4, 300) == 300           # num_neighbors above the rule
    assert E.graphclust_num_neighbors(10 ** 4, 249) == 250
    assert E.graphclust_num_neighbors(50, 80) == 49                   # the clamp to n - 1
    assert E.graphclust_num_neighbors(101, 1, 0.0, 1000.0) == 100
    for n in (0, 1):
        with pytest.raises(Exception):
            E.graphclust_num_neighbors(n)


def test_louvain_labels_against_hand_cases():
    from cellranger_amd import engine as E

    # six barcodes, four used (5, 0, 3, 2 in that order); level 0 lists the nodes 0 .. 3, level 1 lists the communities 0 .. 2 again
    pairs = [(0, 2), (1, 0), (2, 2), (3, 1), (0, 0), (1, 0), (2, 1)]
    use_bcs = np.array([5, 0, 3, 2])
    labels = E.louvain_labels(6, use_bcs, pairs)
    assert labels.dtype == np.int64 and labels.tolist() == [1, 0, 2, 3, 0, 3]          # barcodes 1 and 4 were not used
    assert np.array_equal(labels, R.louvain_labels(6, use_bcs, pairs))
    assert E.louvain_labels(3, np.arange(3), []).tolist() == [0, 0, 0]
    assert E.louvain_labels(3, np.arange(3), [(2, 4), (2, 0)]).tolist() == [0, 0, 5]


def test_relabel_by_size_against_hand_cases():
    from cellranger_amd import engine as E

    # sizes 1: 2, 2: 3, 3: 1 -> 2 becomes 1, 1 becomes 2, 3 becomes 3; label 0 (no member) ranks last
    assert E.relabel_by_size([1, 2, 2, 3, 2, 1]).tolist() == [2, 1, 1, 3, 1, 2]
    # equal sizes keep their ascending order: 1 and 2 with two members each, 3 with three
    assert E.relabel_by_size([1, 2, 3, 3, 2, 1, 3]).tolist() == [2, 3, 1, 1, 3, 2, 1]
    # unused barcodes: label 0 takes part in the ranking as in the reference (sizes 0: 3, 1: 1, 2: 2 -> 0 is first)
    assert E.relabel_by_size([0, 0, 1, 2, 2, 0]).tolist() == [1, 1, 3, 2, 2, 1]
    labels = np.random.RandomState(3).randint(1, 9, 500)
    got = E.relabel_by_size(labels)
    assert np.array_equal(got, 1 + np.argsort(np.argsort(-np.bincount(labels), kind="stable"), kind="stable")[labels])
    sizes = np.bincount(got)[1:]
    assert (np.diff(sizes[:8]) <= 0).all()


def test_write_louvain_edges_lines():
    import io

    from cellranger_amd import engine as E

    buf = io.StringIO()
    assert E.write_louvain_edges(buf, [0, 2, 4, 6], [1, 2, 0, 2, 0, 1]) == 6
    assert buf.getvalue() == "0\t1\n0\t2\n1\t0\n1\t2\n2\t0\n2\t1\n"
    raw = io.BytesIO()
    E.write_louvain_edges(raw, [0, 1, 2], [1, 0])
    assert raw.getvalue() == b"0\t1\n1\t0\n"
