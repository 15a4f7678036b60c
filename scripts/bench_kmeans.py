"""Time of the k-means stage on the device (Context.kmeans, K = 2 .. 10 in one call) against scikit-learn on the same box.
usage (GPU box): python3 scripts/bench_kmeans.py [--repeats 5] [--sizes 10000,100000,1000000] [--pcs 10] [--no-sklearn]
                 rocprofv3 --kernel-trace --stats -d <dir> -- python3 scripts/bench_kmeans.py --trace-run     (a run of its own)
data     seeded Gaussian blobs (12 of them, sd 3 around centres of sd 4: overlapping, so Lloyd runs for tens of rounds), f64, --pcs columns.
call     one warm-up, then --repeats calls of Context.kmeans(X, [2 .. 10]) with the defaults (max_iter 300, tol 1e-4): the host clock
         around the call (minimum, median, maximum) and the n_iter of every K.  The call includes the host's serial mean and variance
         of X, the upload, the seeding, the rounds, the final pass and the downloads.
round    structureless Gaussian noise of the same shape with tol = 0, max_iter = 8 and max_iter = 24 (Lloyd needs far more than 24 rounds
         there; the script checks that no K stopped): the difference of the median call times / 16 is the time of one round of the
         whole list with every K live, with everything outside the rounds cancelled.
bound    the time to stream X once at 6.3 TB/s (the copy rate measured on this part), which one round of the whole list must exceed.
sklearn  KMeans(n_clusters = K, random_state = 0).fit(X) for K = 2 .. 10, one after the other, on the same box's CPU cores; the labels
         of both are compared.
The profiler is off in all of this; --trace-run does one warm-up and one default call at the second size and nothing else."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cellranger_amd import engine as E  # noqa: E402

KS = list(range(2, 11))
STREAM = 6.3e12


def data(n, d):
    rs = np.random.RandomState(7)
    c = rs.normal(0.0, 4.0, (12, d))
    return np.ascontiguousarray(c[rs.randint(12, size=n)] + rs.normal(0.0, 3.0, (n, d)))


def timed(c, X, repeats, **kw):
    c.kmeans(X, KS, **kw)
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        r = c.kmeans(X, KS, **kw)
        ts.append(time.perf_counter() - t0)
    ts = np.sort(ts) * 1e3
    return ts[0], ts[len(ts) // 2], ts[-1], r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sizes", default="10000,100000,1000000")
    ap.add_argument("--pcs", type=int, default=10)
    ap.add_argument("--no-sklearn", action="store_true")
    ap.add_argument("--trace-run", action="store_true")
    a = ap.parse_args()
    sizes = [int(s) for s in a.sizes.split(",")]
    c = E.Context(0)
    if a.trace_run:
        X = data(sizes[min(1, len(sizes) - 1)], a.pcs)
        c.kmeans(X, KS)
        r = c.kmeans(X, KS)
        print("trace run: n=%d d=%d n_iter=%s fit_ms=%.3f" % (len(X), a.pcs, [f["n_iter"] for f in r], r[0]["fit_ms"]))
        c.close()
        return
    for n in sizes:
        X = data(n, a.pcs)
        lo, med, hi, r = timed(c, X, a.repeats)
        iters = [f["n_iter"] for f in r]
        print("n=%d d=%d K=2..10 in one call: call min/median/max %.2f / %.2f / %.2f ms | n_iter %s (sum %d, longest %d) | in LDS: %s" % (
            n, a.pcs, lo, med, hi, iters, sum(iters), max(iters), all(f["in_lds"] for f in r)))
        N = np.random.RandomState(8).normal(0.0, 3.0, (n, a.pcs))
        _, m8, _, r8 = timed(c, N, a.repeats, max_iter=8, tol=0.0)
        _, m24, _, r24 = timed(c, N, a.repeats, max_iter=24, tol=0.0)
        full = all(f["n_iter"] == 24 for f in r24) and all(f["n_iter"] == 8 for f in r8)
        bound = n * a.pcs * 8 / STREAM * 1e6
        print("  one round of the whole list: (%.2f - %.2f ms) / 16 = %.1f us%s | one pass over X at 6.3 TB/s: %.1f us | ratio %.1f" % (
            m24, m8, (m24 - m8) / 16 * 1e3, "" if full else " (SOME K STOPPED EARLY: not a clean figure)", bound, (m24 - m8) / 16 * 1e3 / bound))
        print("  outside the rounds (the max_iter = 8 call less 8 rounds): %.2f ms" % (m8 - (m24 - m8) / 2))
        if not a.no_sklearn:
            from sklearn.cluster import KMeans

            t0 = time.perf_counter()
            same = []
            for f in r:
                km = KMeans(n_clusters=f["n_clusters"], random_state=0).fit(X)
                same.append(bool(np.array_equal(km.labels_, f["labels"])) and km.n_iter_ == f["n_iter"])
            t_sk = time.perf_counter() - t0
            print("  scikit-learn, the nine fits one after the other: %.2f s | ratio to the device call %.0f | labels and n_iter equal per K: %s" % (
                t_sk, t_sk * 1e3 / med, same))
    c.close()


if __name__ == "__main__":
    main()
