"""Time of the exact k-nearest-neighbour query on the device (Context.knn, the hot path of RUN_GRAPH_CLUSTERING) against scikit-learn's
BallTree on the same box.
usage (GPU box): python3 scripts/bench_knn.py [--repeats 3] [--pcs 10] [--no-sklearn] [--force-million]
data     seeded Gaussian blobs (12 of them, sd 3 around centres of sd 4), f64, --pcs columns; k by split()'s rule: 250 neighbours at
         10 000 cells, 370 at 100 000, 490 at 1 000 000.
figure   every size is measured by a child process of its own with its own time limit (a child that fails or runs into its limit ends
         the script: nothing more is started on the device).  One warm-up call, then --repeats calls of Context.knn(X, k) over all
         rows; the host clock around the call (minimum, median, maximum), which includes the finiteness check and packing of X on the
         host, the upload and the download of the three outputs; the device time of the pass over the candidates (select) and of the
         final sort from events around the two kernels; pairs per second = rows^2 / that time; the share of the final sort in the
         device time; compactions per query tile and pairs appended per query.
million  1 000 000 cells are measured only when 100 times the call at 100 000 predicts under a minute (the pairs grow 100-fold; k grows
         from 370 to 490 on top), as 67 calls of 15 000 query rows -- the reference's chunks, which bound the host output; the script
         says which it was.
sklearn  BallTree(X, leaf_size = 40) build plus query(X, k + 1) on the same box's CPU (one thread, as the reference's chunk jobs run
         it) in a child with a time limit, and whether its [:, 1:] equals the device's arrays; "not timed" where scikit-learn does not
         import or the limit ran out.
What binds the pass is not measured here: no counters are taken."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CHUNK = 15000
LIMITS = {10000: 120, 100000: 240, 1000000: 420}       # seconds per child
SKLEARN_LIMIT = 200


def data(n, d):
    rs = np.random.RandomState(7)
    c = rs.normal(0.0, 4.0, (12, d))
    return np.ascontiguousarray(c[rs.randint(12, size=n)] + rs.normal(0.0, 3.0, (n, d)))


def child_device(n, d, repeats, out_path):
    from cellranger_amd import engine as E

    X = data(n, d)
    k = E.graphclust_num_neighbors(n)
    c = E.Context(0)
    res = dict(n=n, d=d, k=k)
    if n <= 100000:
        c.knn(X, k)
        calls, sel, srt = [], [], []
        for _ in range(repeats):
            t0 = time.perf_counter()
            r = c.knn(X, k)
            calls.append((time.perf_counter() - t0) * 1e3)
            sel.append(r["select_ms"])
            srt.append(r["sort_ms"])
        res.update(calls=sorted(calls), select_ms=float(np.median(sel)), sort_ms=float(np.median(srt)), compactions=r["compactions"],
                   query_tiles=r["query_tiles"], survivors=r["survivors"], capacity=r["capacity"], in_lds=r["in_lds"], pairs=r["pairs_evaluated"])
        np.save(out_path, r["indices"][:2000])
    else:                                               # the reference's chunks: 15 000 query rows a call
        c.knn(X, k, query_start=0, n_queries=1000)
        t0 = time.perf_counter()
        sel = srt = 0.0
        pairs = comp = tiles = surv = 0
        first = None
        for q0 in range(0, n, CHUNK):
            r = c.knn(X, k, query_start=q0, n_queries=min(CHUNK, n - q0))
            sel, srt, pairs = sel + r["select_ms"], srt + r["sort_ms"], pairs + r["pairs_evaluated"]
            comp, tiles, surv = comp + r["compactions"], tiles + r["query_tiles"], surv + r["survivors"]
            first = r["indices"][:2000] if first is None else first
        res.update(calls=[(time.perf_counter() - t0) * 1e3], select_ms=sel, sort_ms=srt, compactions=comp, query_tiles=tiles, survivors=surv,
                   capacity=r["capacity"], in_lds=r["in_lds"], pairs=pairs, n_calls=-(-n // CHUNK))
        np.save(out_path, first)
    c.close()
    print("RESULT " + json.dumps(res))


def child_sklearn(n, d, dev_path):
    os.environ.setdefault("OMP_NUM_THREADS", "1")
    from sklearn.neighbors import BallTree

    from cellranger_amd import _lib  # noqa: F401  (the rule on the host, no device)
    from cellranger_amd import engine as E

    X = data(n, d)
    k = E.graphclust_num_neighbors(n)
    t0 = time.perf_counter()
    tree = BallTree(X, leaf_size=40)
    t1 = time.perf_counter()
    _, ind = tree.query(X, k + 1)
    t2 = time.perf_counter()
    dev = np.load(dev_path)
    print("RESULT " + json.dumps(dict(build_s=t1 - t0, query_s=t2 - t1, equal=bool(np.array_equal(ind[:len(dev), 1:], dev)))))


def run_child(args, limit):
    """-> the child's RESULT dict, or None when it ran into its limit; any other failure ends the script"""
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        return None
    if r.returncode != 0:
        sys.stdout.write(r.stdout + r.stderr)
        raise SystemExit("a child failed (exit %d): nothing more is started" % r.returncode)
    for line in r.stdout.splitlines():
        if line.startswith("RESULT "):
            return json.loads(line[7:])
    raise SystemExit("a child printed no result")


def report(res):
    calls, n = res["calls"], res["n"]
    dev_ms = res["select_ms"] + res["sort_ms"]
    how = "%d calls of %d query rows" % (res["n_calls"], CHUNK) if "n_calls" in res else "one call over all rows, min/median/max of the repeats"
    print("n=%d d=%d k=%d (%s): call %s ms | device: select %.2f ms + final sort %.2f ms, the sort's share %.1f %% | "
          "%.3g pairs: %.3g pairs/s of the select pass, %.3g of the call | buffer %d pairs, in LDS: %s | compactions per query tile %.1f | "
          "pairs appended per query %.0f (k + 1 = %d)" % (
              n, res["d"], res["k"], how, " / ".join("%.2f" % t for t in (calls[0], calls[len(calls) // 2], calls[-1])) if len(calls) > 1 else "%.2f" % calls[0],
              res["select_ms"], res["sort_ms"], 100.0 * res["sort_ms"] / dev_ms, res["pairs"], res["pairs"] / (res["select_ms"] * 1e-3),
              res["pairs"] / (calls[len(calls) // 2] * 1e-3), res["capacity"], res["in_lds"], res["compactions"] / res["query_tiles"],
              res["survivors"] / float(n), res["k"] + 1))
    sys.stdout.flush()
    return calls[len(calls) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--pcs", type=int, default=10)
    ap.add_argument("--no-sklearn", action="store_true")
    ap.add_argument("--force-million", action="store_true")
    ap.add_argument("--child-device", type=int, default=0)
    ap.add_argument("--child-sklearn", type=int, default=0)
    ap.add_argument("--scratch", default="")
    a = ap.parse_args()
    if a.child_device:
        return child_device(a.child_device, a.pcs, a.repeats, a.scratch)
    if a.child_sklearn:
        return child_sklearn(a.child_sklearn, a.pcs, a.scratch)
    import tempfile

    tmp = tempfile.mkdtemp(prefix="bench_knn_")
    common = ["--pcs", str(a.pcs), "--repeats", str(a.repeats)]
    median = {}
    sizes = [10000, 100000]
    for n in sizes:
        path = os.path.join(tmp, "dev_%d.npy" % n)
        res = run_child(["--child-device", str(n), "--scratch", path] + common, LIMITS[n])
        if res is None:
            raise SystemExit("n=%d: the device child ran into its limit of %d s: nothing more is started" % (n, LIMITS[n]))
        median[n] = report(res)
        if n == 100000:
            predicted = 100.0 * median[n] * 1e-3
            go = predicted < 60.0 or a.force_million
            print("  1 000 000 cells: 100 x the call at 100 000 predicts %.1f s, %s a minute: %s" % (
                predicted, "under" if predicted < 60.0 else "NOT under", "measured below" if go else "not measured"))
            if go:
                sizes.append(1000000)
        if a.no_sklearn:
            print("  scikit-learn: not timed (--no-sklearn)")
            continue
        try:
            import sklearn  # noqa: F401
        except ImportError:
            print("  scikit-learn: not timed (it does not import here)")
            continue
        if n > 100000:
            print("  scikit-learn BallTree: not timed (100 000 cells take the better part of a minute on one thread, and the work grows "
                  "faster than the rows: beyond the limit of %d s)" % SKLEARN_LIMIT)
            continue
        sk = run_child(["--child-sklearn", str(n), "--scratch", path] + common, SKLEARN_LIMIT)
        if sk is None:
            print("  scikit-learn BallTree: not timed (build + query did not end within %d s on one thread)" % SKLEARN_LIMIT)
        else:
            print("  scikit-learn BallTree, one thread: build %.2f s + query(X, k + 1) %.2f s = %.2f s | ratio to the device call %.0f | "
                  "its [:, 1:] equals the device's indices on the first 2000 rows: %s" % (
                      sk["build_s"], sk["query_s"], sk["build_s"] + sk["query_s"], (sk["build_s"] + sk["query_s"]) * 1e3 / median[n], sk["equal"]))
        sys.stdout.flush()


if __name__ == "__main__":
    main()
