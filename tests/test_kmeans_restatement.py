"""CPU checks of the numpy restatement of RUN_KMEANS (tests/kmeans_numpy.py) against tests/golden/kmeans_reference.npz, which
scripts/make_kmeans_golden.py recorded from scikit-learn 1.7.2's KMeans(n_clusters = K, random_state = 0) (init = array, n_init = 1 for
the fixture with a far-away centre): labels, centres, inertia, n_iter_, the seeding indices of sklearn.cluster.kmeans_plusplus under the
same state.  The recorder rejected every fixture whose outcome hangs on a rounding (its docstring has the rules), so the integers are
asserted equal: labels, n_iter, the strict flag, sizes, the relabelled clusters, the seeding indices.  Floats are held to
16 x the largest movement of the quantity between three orders of the sums over cells (cell order, 256-cell partials, reverse), read
from the file: scikit-learn's own order depends on its thread count.  The movement is relative for inertia, wss and the score, and
absolute against the data's largest magnitude for the centres.

compute_db_index and relabel_by_size are restated (the reference's modules need numexpr): they are pinned here by hand-computed cases
and checked against scipy.spatial.distance.pdist and np.bincount / np.argsort.  The seed hook of the library equals
np.random.RandomState(seed) bit for bit."""
import functools
import os

import numpy as np
import pytest

import kmeans_numpy as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(name, k) for name, f in R.FIXTURES.items() for k in f["ks"]]


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(os.path.join(ROOT, "tests", "golden", "kmeans_reference.npz")) as z:
        return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def fixture(name):
    """-> (X, init, max_iter) of the fixture as the recorder settled on it"""
    return R.fixture_data(name, int(golden()[name + "/seed"]))


def bounds():
    g = golden()
    return {q: 16.0 * float(g["move_" + q]) for q in ("centers", "inertia", "wss", "score")}


def check_against_golden(name, k, got, who):
    """the equalities and the float bounds every implementation is held to; prints each figure before it asserts"""
    g = golden()
    p = "%s/k%d/" % (name, k)
    b = bounds()
    scale = float(g[p + "scale"])
    worst = dict(centers=float(np.abs(got["centers"] - g[p + "centers"]).max()) / scale,
                 inertia=abs(got["inertia"] - float(g[p + "inertia"])) / float(g[p + "inertia"]) if g[p + "inertia"] else abs(got["inertia"]),
                 wss=float(np.abs(got["wss"] - g[p + "wss"]).max()) / float(g[p + "wss"].max()) if g[p + "wss"].max() else float(np.abs(got["wss"]).max()),
                 score=abs(got["db_score"] - float(g[p + "db_score"])) / float(g[p + "db_score"]) if g[p + "db_score"] else abs(got["db_score"]))
    print(who, name, "K", k, "n_iter", got["n_iter"], "differences", worst, "bounds", b)
    assert np.array_equal(got["labels"], g[p + "labels"].astype(np.int32))
    assert np.array_equal(got["clusters"], g[p + "clusters"].astype(np.int32))
    assert (got["n_iter"], bool(got["strict"]), got["relocations"]) == (int(g[p + "n_iter"]), bool(g[p + "strict"]), int(g[p + "relocations"]))
    assert np.array_equal(np.asarray(got["sizes"], np.uint64), g[p + "sizes"])
    for q, v in worst.items():
        assert v <= b[q], (q, v, b[q])


def test_golden_file_covers_the_table_and_the_special_cases():
    g = golden()
    shapes = {(f["n"], f["d"]): set() for f in R.FIXTURES.values()}
    for name, f in R.FIXTURES.items():
        X, _, _ = fixture(name)
        assert X.shape == (f["n"], f["d"])
        shapes[X.shape] |= set(f["ks"])
        for k in f["ks"]:
            assert len(g["%s/k%d/labels" % (name, k)]) == f["n"] and g["%s/k%d/centers" % (name, k)].shape == (k, f["d"])
    assert shapes[(2, 1)] >= {1, 2} and shapes[(300, 1)] >= {2, 5, 10} and shapes[(4099, 128)] >= {64}
    for n in (255, 256, 257):
        assert shapes[(n, 10)] >= {1, 2, 5, 10}
    assert shapes[(1000, 10)] >= set(range(2, 11)) and shapes[(4099, 10)] >= {2, 5, 10} and shapes[(5000, 50)] >= {2, 5, 10}
    assert g["n_equals_k/k5/n_iter"] >= 1 and R.FIXTURES["n_equals_k"]["n"] == 5
    assert (g["three_points/k5/sizes"] == 0).sum() == 2 and g["three_points/k5/inertia"] == 0.0      # potential 0, weight-0 clusters
    assert g["far_init/k3/relocations"] == 1 and len(g["far_init/k3/seeds"]) == 0
    assert g["round_limit/k10/n_iter"] == 2 and not g["round_limit/k10/strict"]
    assert g["equal_sizes/k2/sizes"].tolist() == [100, 100]
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "kmeans_reference.npz")) < (1 << 20)
    assert all(0.0 < v < 1e-12 for v in bounds().values())


@functools.lru_cache(maxsize=None)
def restated(name, k):
    X, init, max_iter = fixture(name)
    return R.fit(X, k, 0, init, max_iter)


@pytest.mark.parametrize("name,k", CASES)
def test_restatement_equals_the_golden_file(name, k):
    got = restated(name, k)
    check_against_golden(name, k, got, "restatement")
    seeds = golden()["%s/k%d/seeds" % (name, k)]
    assert (got["seeds"] is None and not len(seeds)) or np.array_equal(got["seeds"], seeds)


def test_weight_zero_cluster_takes_the_heaviest_row():
    """three distinct points, five centres: the two clusters that stay empty are not left at the origin"""
    got = restated("three_points", 5)
    pts = {(0.0, 0.0), (6.0, 0.0), (0.0, 12.0)}
    assert got["relocations"] == 0 and {tuple(c) for c in got["centers"][got["sizes"] > 0]} == pts
    heavy = int(np.argmax(got["sizes"]))
    for j in np.flatnonzero(got["sizes"] == 0):
        if j > heavy:
            assert np.array_equal(got["centers"][j], got["centers"][heavy])


def test_db_index_by_hand_and_against_scipy():
    from scipy.spatial.distance import pdist, squareform

    # two clusters 5 apart with scatter 2 and 3: both rows are (2 + 3) / 5
    assert R.db_index(np.array([[0.0, 0.0], [3.0, 4.0]]), [8.0, 18.0], [2, 2]) == 1.0
    # the clamp at 1e-3 and a count of 0 taken as 1
    assert R.db_index(np.array([[0.0], [1e-4]]), [4.0, 4.0], [4, 0]) == 3.0 / 1e-3
    assert R.db_index(np.array([[7.0]]), [4.0], [4]) == 0.0
    rs = np.random.RandomState(5)
    X = rs.normal(size=(200, 7))
    labels = rs.randint(6, size=200).astype(np.int32)
    labels[labels == 4] = 3      # an empty cluster
    centers = rs.normal(size=(6, 7))
    centers[5] = centers[0] + 1e-5      # under the clamp
    wss, counts = R.db_sums(X, centers, labels)
    # compute_db_index as the reference writes it, on scipy's distances
    dist = squareform(pdist(centers))
    dist[np.abs(dist) < 1e-3] = 1e-3
    w, c = np.zeros(6), np.zeros(6)
    for i in range(200):
        w[labels[i]] += np.square(X[i, :] - centers[labels[i], :]).sum()
        c[labels[i]] += 1
    c[c == 0] = 1
    s = np.sqrt(w / c)
    mix = (s + s[:, np.newaxis]) / dist
    np.fill_diagonal(mix, 0.0)
    want = np.max(mix, axis=1).sum() / 6
    assert counts.tolist() == np.bincount(labels, minlength=6).tolist() and counts[4] == 0
    assert np.allclose(wss, w, rtol=1e-13) and abs(R.db_index(centers, wss, counts) - want) <= 1e-13 * want


def test_relabel_by_size_by_hand_and_against_numpy():
    # sizes 2, 3, 1: cluster 1 (0-based) becomes 1, cluster 0 becomes 2, cluster 2 becomes 3
    assert R.relabel_by_size(np.array([0, 0, 1, 1, 1, 2]), 3).tolist() == [2, 2, 1, 1, 1, 3]
    # equal sizes keep their order; an empty cluster ranks behind index 0 of the bincount and is never used
    assert R.relabel_by_size(np.array([1, 0, 1, 0]), 2).tolist() == [2, 1, 2, 1]
    assert R.relabel_by_size(np.array([2, 2, 0]), 3).tolist() == [1, 1, 2]
    rs = np.random.RandomState(9)
    for k in (2, 10, 64):
        labels = rs.randint(k, size=500)
        one_based = labels + 1
        order = np.argsort(np.argsort(-np.bincount(one_based), kind="stable"), kind="stable")      # the reference's line, with the stable kind
        assert np.array_equal(R.relabel_by_size(labels, k), 1 + order[one_based])
    assert np.array_equal(R.relabel_by_size(golden()["equal_sizes/k2/labels"].astype(np.int32), 2), golden()["equal_sizes/k2/labels"].astype(np.int32) + 1)


@pytest.mark.parametrize("seed", [0, 12345])
@pytest.mark.parametrize("n,k", [(2, 2), (300, 5), (4099, 10), (100001, 64)])
def test_seed_hook_equals_numpy(seed, n, k):
    from cellranger_amd import build, engine as E

    build.build()
    u, first = E.kmeans_seed_draws(seed, n, k)
    rs = np.random.RandomState(seed)
    T = 2 + int(np.log(k))
    state = rs.get_state()
    want_first = rs.choice(n, p=np.ones(n) / np.ones(n).sum())      # numpy's own choice() and uniform(), the calls scikit-learn makes
    probe = np.random.RandomState()
    probe.set_state(state)
    want = [probe.random_sample()] + [v for _ in range(k - 1) for v in rs.uniform(size=T)]
    assert len(u) == 1 + (k - 1) * T and u.tobytes() == np.array(want).tobytes() and first == want_first
    ru, rf = R.seed_draws(seed, n, k)
    assert u.tobytes() == ru.tobytes() and first == rf and E.kmeans_trials(k) == T == R.trials(k)
