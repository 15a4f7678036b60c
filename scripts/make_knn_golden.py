#!/usr/bin/env python
"""Record tests/golden/knn_reference.npz: scikit-learn 1.7.2's BallTree(x, leaf_size = 40).query(x, k + 1)[.][:, 1:] -- what
compute_nearest_neighbors (analysis/graphclust.py:39-62) returns -- for every fixture of tests/knn_numpy.py but mid_5000.

Per fixture <name>_rows (a seeded sample of the rows, rows 0 and n - 1 always, so that the file stays small; never the fixture itself
is cut), <name>_ind i32[rows, k] and <name>_dist f64[rows, k].  Leaf size 2 must give the same arrays on every tie-free fixture (the
tree does not matter) and the same distances on the tied ones.

A fixture meant to be tie-free is REJECTED when any of its rows has two equal d2 among its first k + 2; at most 1 in 8 may be
(the count is printed; the seed of a rejected fixture is to be changed in tests/knn_numpy.py).  A tied fixture is rejected when BallTree's
DISTANCES differ from the restatement's in any bit.

    python scripts/make_knn_golden.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import knn_numpy as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "knn_reference.npz")
ENTRIES = 2500         # rows * k stored per fixture, about
SAMPLE_SEED = 20261020


def sample_rows(n, k):
    m = max(2, min(n, ENTRIES // k))
    if m >= n:
        return np.arange(n)
    rs = np.random.RandomState(SAMPLE_SEED + n + k)
    inner = rs.choice(np.arange(1, n - 1), m - 2, replace=False)
    return np.sort(np.concatenate([[0, n - 1], inner]))


def main():
    import sklearn
    from sklearn.neighbors import BallTree

    assert sklearn.__version__ == "1.7.2", "the reference is scikit-learn 1.7.2, this is %s" % sklearn.__version__
    out, tie_free, rejected, smallest_gap = {}, 0, [], np.inf
    for name, f in R.FIXTURES.items():
        if name in R.NOT_IN_GOLDEN:
            continue
        x, k = R.used(name), f["k"]
        dist, ind = BallTree(x, leaf_size=40).query(x, k + 1)
        dist2, ind2 = BallTree(x, leaf_size=2).query(x, k + 1)
        r_ind, r_dist, _ = R.expected(name)
        if f["tied"]:
            if not (np.array_equal(dist[:, 1:], r_dist) and np.array_equal(dist2[:, 1:], r_dist)):
                raise SystemExit("%s: BallTree's distances differ from the restatement's" % name)
        else:
            tie_free += 1
            n = len(x)
            first = np.sort(np.concatenate([R.d2_rows(x, lo, min(lo + 512, n)) for lo in range(0, n, 512)]), axis=1)[:, :k + 2]
            gaps = np.diff(first, axis=1)
            if (gaps == 0).any():
                rejected.append(name)
                continue
            smallest_gap = min(smallest_gap, float(gaps.min()))
            assert np.array_equal(ind, ind2) and np.array_equal(dist, dist2), "%s: the leaf size moved the answer" % name
            assert np.array_equal(ind[:, 1:], r_ind) and np.array_equal(dist[:, 1:], r_dist), "%s: the restatement differs from BallTree" % name
        rows = sample_rows(len(x), k)
        out[name + "_rows"] = rows.astype(np.int32)
        out[name + "_ind"] = ind[rows, 1:].astype(np.int32)
        out[name + "_dist"] = dist[rows, 1:]
    print("tie-free fixtures: %d, rejected: %d %s, smallest gap of d2 among the first k + 2: %.3g" % (tie_free, len(rejected), rejected, smallest_gap))
    if rejected:
        raise SystemExit("change the seed of %s in tests/knn_numpy.py%s" % (rejected, "" if 8 * len(rejected) <= tie_free else " (more than 1 in 8)"))
    np.savez_compressed(OUT, **out)
    print("%s: %d bytes" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
