"""Records tests/golden/merge_clusters_reference.npz: for every fixture of tests/merge_clusters_numpy.py the loop of
stages/analyzer/merge_clusters join() run with the stage's own tools -- scipy's linkage(medoids, "complete"), pandas'
groupby("cluster").apply(lambda x: x.median(axis=0)), the cells of a leaf in cell order (np.flatnonzero(labels == leaf)) -- and
tests/sseq_numpy.py as the test.  Stored per fixture: the medoids and Z of every iteration, the step log (leaves, their initial groups,
n_de, merged, skipped), the smallest adjusted p of every test, the counts and the final labels.  Data only.

A fixture is rejected, named, and replaced by its next seed when a comparison would hang on a rounding:
  - two pairwise medoid distances or two merge heights of an iteration within 1e-9 relative (the dendrogram would depend on a tie rule);
  - an adjusted p-value of a test within 1e-6 relative of 0.05 (n_de would depend on the order of a sum);
  - the rejection of scripts/make_sseq_golden.py fires in a test (an exact-test term next to the observed one, an asymptotic test on
    the median).
The number of rejected fixtures is printed and stored.

    python scripts/make_merge_clusters_golden.py        (scipy 1.15.3, pandas 2.3.3)"""
import os
import sys
import warnings

import numpy as np
import pandas as pd
import scipy
from scipy.cluster.hierarchy import linkage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import merge_clusters_numpy as M  # noqa: E402
import sseq_numpy as S  # noqa: E402


class Rejected(Exception):
    pass


def close(values, rel):
    v = np.sort(np.asarray(values, np.float64))
    return len(v) > 1 and bool(np.any(np.diff(v) <= rel * np.abs(v[1:])))


def pandas_medians(pca, labels, n_clusters):
    df = pd.DataFrame(pca)
    df["cluster"] = labels
    warnings.simplefilter("ignore", FutureWarning)      # pandas 2.3 announces a change of apply() on the grouping column
    return df.groupby("cluster").apply(lambda x: x.median(axis=0)).to_numpy()[:, :-1]


def scipy_linkage(medoids):
    K = len(medoids)
    D = np.sqrt(((medoids[:, None, :] - medoids[None, :, :]) ** 2).sum(axis=2))[np.triu_indices(K, 1)]
    hc = linkage(medoids, "complete")
    if close(D, 1e-9) or close(hc[:, 2], 1e-9):
        raise Rejected("two medoid distances or merge heights within 1e-9")
    return hc


def record(name, bump):
    x, pca, labels = M.fixture(name, bump)

    def stage_test(a, b, cells0, cells1):      # the stage's submatrix: the cells of both leaves in cell order
        sub = x[:, np.concatenate((cells0, cells1))]
        lab = np.array([1] * len(cells0) + [2] * len(cells1), np.int32)
        P = S.compute_params(sub)
        o = S.diffexp(sub, P, lab, 2)
        q = o["adjusted_p_values"][0]
        if np.any(np.abs(q - M.DE_THRESHOLD) <= 1e-6 * M.DE_THRESHOLD):
            raise Rejected("an adjusted p-value within 1e-6 of %g" % M.DE_THRESHOLD)
        if np.any(o["min_gap"][0] < 1e-6):
            raise Rejected("an exact-test term %.3g from the observed one" % o["min_gap"][0].min())
        big = o["below_median"][0] != 255
        T = (o["sums_in"][0] + o["sums_out"][0]).astype(np.float64)
        if big.any() and np.min(np.abs((o["sums_in"][0][big] + 0.5) / T[big] - o["median"][0][big])) < 1e-9:
            raise Rejected("an asymptotic test on the median")
        return dict(n_de=int(np.sum(q < M.DE_THRESHOLD)), min_q=float(q.min()), adjusted_p_values=q)

    trace = []
    o = M.merge_clusters(x, pca, labels, medians=pandas_medians, linkage=scipy_linkage, test=stage_test, trace=trace)
    return o, trace


def main():
    out, rejected = {}, []
    for name in sorted(M.FIXTURES):
        bump = 0
        while True:
            try:
                o, trace = record(name, bump)
                break
            except (Rejected, ValueError) as e:
                rejected.append("%s (seed bump %d): %s" % (name, bump, e))
                bump += 1
                if bump > 4:
                    raise SystemExit("fixture %s: five seeds rejected" % name)
        tab, flat, off = M.steps_table(o["steps"])
        its = [t for t in trace if t[0] == "iteration"]
        out[name + ".bump"] = np.int64(bump)
        out[name + ".labels"] = o["labels"]
        out[name + ".steps"], out[name + ".step_groups"], out[name + ".step_group_offsets"] = tab, flat, off
        out[name + ".min_q"] = np.array([t[1] for t in trace if t[0] == "test"])
        out[name + ".counts"] = np.array([o[k] for k in ("n_tests", "n_skipped", "n_merges", "n_iterations", "n_clusters_in", "n_clusters_out")], np.int64)
        for i, (_, medoids, hc) in enumerate(its):
            out["%s.medoids.%d" % (name, i)], out["%s.Z.%d" % (name, i)] = medoids, hc
        print("%-16s seed bump %d: %d -> %d clusters, %d tests, %d skipped, %d merges, %d iterations" % (
            name, bump, o["n_clusters_in"], o["n_clusters_out"], o["n_tests"], o["n_skipped"], o["n_merges"], o["n_iterations"]))
    for r in rejected:
        print("rejected: " + r)
    print("%d fixtures rejected of %d" % (len(rejected), len(M.FIXTURES)))
    out["n_rejected"] = np.int64(len(rejected))
    out["versions"] = np.array(["scipy " + scipy.__version__, "pandas " + pd.__version__, "numpy " + np.__version__])
    path = os.path.join(ROOT, "tests", "golden", "merge_clusters_reference.npz")
    np.savez_compressed(path, **out)
    print("%s: %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
