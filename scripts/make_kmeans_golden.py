"""Records tests/golden/kmeans_reference.npz on the CPU from scikit-learn 1.7.2: for every fixture of tests/kmeans_numpy.py and every K of
it, labels, centres, inertia and n_iter_ of KMeans(n_clusters = K, random_state = 0) (KMeans(init = array, n_init = 1) where the
fixture gives centres), the seeding indices of sklearn.cluster.kmeans_plusplus under the same state, and the restated
compute_db_index / relabel_by_size on scikit-learn's labels and centres.

    python scripts/make_kmeans_golden.py

A fixture whose outcome hangs on a rounding is REJECTED, printed, and replaced by the next seed of the same shape: a point whose two
nearest centres differ by less than 1e-9 relative at any round, a seeding draw within 1e-9 relative of a boundary of the cumulative
sum, two candidates' potentials within 1e-9 relative, sum(shift^2) within 1e-6 relative of tol, or labels that differ between the
three sum orders.  More than one rejection in ten fixtures, or a fixture left without a record, fails the run.  The file also holds,
per fit, how far the restatement's floats move between the three orders of the sums over cells -- the per-cluster sums of a round, the per-cluster wss and the inertia,
each in cell order, as 256-cell partials and in reverse --, and as `move_*` the largest movement of each quantity over all fits: the
tests allow 16 times that against scikit-learn's values, whose own order depends on its thread count."""
import os
import sys
import warnings

import numpy as np
import sklearn
from sklearn.cluster import KMeans, kmeans_plusplus

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import kmeans_numpy as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "kmeans_reference.npz")
SEEDED = ("blobs", "equal_sizes")


def record_fit(X, k, init, max_iter):
    """-> (record dict, None) or (None, the reason of the rejection)"""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        km = KMeans(n_clusters=k, random_state=0, max_iter=max_iter, **({} if init is None else dict(init=init.copy(), n_init=1))).fit(X.copy())
    diag = {}
    fits = {o: R.fit(X, k, 0, init, max_iter, order=o, diag=diag if o == "cell" else None) for o in R.ORDERS}
    a = fits["cell"]
    for name, bound in (("gap", 1e-9), ("draw", 1e-9), ("pot", 1e-9), ("tol", 1e-6)):
        if diag.get(name, np.inf) < bound:
            return None, "%s %.3g below %.0e" % (name, diag[name], bound)
    for o in R.ORDERS[1:]:
        if not np.array_equal(fits[o]["labels"], a["labels"]) or fits[o]["n_iter"] != a["n_iter"]:
            return None, "the labels depend on the sum order (%s)" % o
    seeds = None
    if init is None:
        Xc = X - X.mean(axis=0)
        seeds = kmeans_plusplus(Xc, k, random_state=0)[1]
        assert np.array_equal(seeds, a["seeds"]), ("seeding differs from scikit-learn", seeds, a["seeds"])
    assert np.array_equal(km.labels_, a["labels"]) and km.n_iter_ == a["n_iter"], ("the restatement differs from scikit-learn", k, km.n_iter_, a["n_iter"])
    labels, centers = km.labels_.astype(np.int32), km.cluster_centers_
    wss, sizes = R.db_sums(X, centers, labels)
    scale = float(np.abs(X).max())
    mv = dict(centers=0.0, inertia=0.0, wss=0.0, score=0.0)
    for o in R.ORDERS[1:]:
        b = fits[o]
        mv["centers"] = max(mv["centers"], float(np.abs(b["centers"] - a["centers"]).max()) / scale)
        mv["inertia"] = max(mv["inertia"], abs(b["inertia"] - a["inertia"]) / a["inertia"] if a["inertia"] else 0.0)
        mv["wss"] = max(mv["wss"], float(np.abs(b["wss"] - a["wss"]).max()) / a["wss"].max() if a["wss"].max() else 0.0)
        mv["score"] = max(mv["score"], abs(b["db_score"] - a["db_score"]) / a["db_score"] if a["db_score"] else 0.0)
    rec = dict(labels=labels.astype(np.uint8), centers=centers, inertia=km.inertia_, n_iter=km.n_iter_, strict=a["strict"], relocations=a["relocations"],
               seeds=np.zeros(0, np.int64) if seeds is None else seeds, wss=wss, sizes=sizes, db_score=R.db_index(centers, wss, sizes),
               clusters=R.relabel_by_size(labels, k).astype(np.uint8), scale=scale, tol=a["tol"],
               **{"move_" + q: v for q, v in mv.items()})
    return rec, None


def main():
    assert sklearn.__version__ == "1.7.2", "the golden file is scikit-learn 1.7.2's; found " + sklearn.__version__
    out, rejected, done = {}, 0, 0
    for name, f in R.FIXTURES.items():
        for seed in range(8 if f["kind"] in SEEDED else 1):
            X, init, max_iter = R.fixture_data(name, seed)
            recs, why = {}, None
            for k in f["ks"]:
                recs[k], why = record_fit(X, k, init, max_iter)
                if why:
                    why = "K = %d: %s" % (k, why)
                    break
            if why is None:
                break
            rejected += 1
            print("REJECTED %s seed %d: %s" % (name, seed, why))
        assert why is None, "no fixture for " + name
        done += 1
        out[name + "/seed"] = np.int64(seed)
        for k, rec in recs.items():
            for q, v in rec.items():
                out["%s/k%d/%s" % (name, k, q)] = np.asarray(v)
            print("%-14s K = %2d: n_iter %3d strict %d relocations %d inertia %.6g score %.6g; movement centres %.2g inertia %.2g wss %.2g score %.2g" % (
                name, k, rec["n_iter"], rec["strict"], rec["relocations"], rec["inertia"], rec["db_score"], rec["move_centers"], rec["move_inertia"],
                rec["move_wss"], rec["move_score"]))
    assert rejected * 10 <= done, "%d rejections for %d fixtures" % (rejected, done)
    # what the special cases are there for
    assert out["far_init/k3/relocations"] == 1 and out["round_limit/k10/n_iter"] == 2 and not out["round_limit/k10/strict"]
    assert len(set(out["equal_sizes/k2/sizes"].tolist())) == 1 and (out["three_points/k5/sizes"] == 0).any()
    for q in ("centers", "inertia", "wss", "score"):      # the largest movement per quantity
        out["move_" + q] = np.float64(max(float(v) for key, v in out.items() if key.endswith("/move_" + q)))
        print("largest movement of %s: %.3g" % (q, out["move_" + q]))
    np.savez_compressed(OUT, **out)
    print("%s: %d fixtures, %d rejected, %d bytes" % (OUT, done, rejected, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
