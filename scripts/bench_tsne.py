"""Time of RUN_TSNE on the device (engine.run_tsne's phases: Context.knn, Context.tsne_affinities, Context.tsne) against two CPU
yardsticks on the same box.
usage (GPU box): python3 scripts/bench_tsne.py [--iters 20] [--pcs 10] [--no-cpu] [--force-million]
data     seeded Gaussian blobs (12 of them, sd 3 around centres of sd 4), f64, --pcs columns, perplexity 30 (K = 90), 2 output dimensions.
figure   every size is measured by a child process of its own with its own time limit (a child that fails or runs into its limit ends
         the script: nothing more is started on the device).  The phases by the host clock: normalisation, the neighbour search in
         calls of 15 000 rows, the affinities (search_ms and csr_ms are its device times), then Context.tsne for --iters iterations
         after a warm-up call of 2: loop_ms (events around the loop) / iterations = time per iteration; repulse_ms = device time of the
         repulsion launches of the last iteration; pairs per second = N (N - 1) / repulse_ms; against the 39.3e12 unfused f64
         operations per second the part can reach (half its 78.6 Tflop/s vector peak, the README's figure) at OPS_PER_PAIR operations
         a pair in 2 dimensions, the division counted as one.
million  the stage's 1000 iterations at 1 000 000 cells are 100 times those at 100 000.  When that prediction is under ten minutes the
         size is run like the others; otherwise only 2 iterations are run there (when they are predicted under two minutes) and the
         full run is an EXTRAPOLATION, which the script says.
cpu      scikit-learn's TSNE(method="barnes_hut", angle=0.5) -- a DIFFERENT algorithm (a tree, float32 neighbours, its own start) --
         for its minimum of 250 iterations with the box's 16 threads, and one iteration of the numpy restatement tests/tsne_numpy.py
         (the same algorithm as the device's, one thread of numpy), at 10 000 cells, each in a child with a time limit.
What binds the repulsion kernel is not measured here: no counters are taken."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CHUNK = 15000
PERPLEXITY = 30
OPS_PER_PAIR = 14        # 2 sub, 2 mul, 1 add (d2); 1 add, 1 div (q); 1 add (z); 1 mul (q q); 2 mul, 2 add (neg); the select for i = j
UNFUSED_PEAK = 39.3e12
LIMITS = {10000: 180, 100000: 300, 1000000: 560}       # seconds per child
CPU_LIMIT = 300


def data(n, d):
    rs = np.random.RandomState(7)
    c = rs.normal(0.0, 4.0, (12, d))
    return np.ascontiguousarray(c[rs.randint(12, size=n)] + rs.normal(0.0, 3.0, (n, d)))


def child_device(n, d, iters):
    from cellranger_amd import engine as E

    X = data(n, d)
    K = int(3 * PERPLEXITY)
    c = E.Context(0)
    t0 = time.perf_counter()
    x = np.ascontiguousarray(E.tsne_normalize(X))
    t1 = time.perf_counter()
    ind, dist = np.zeros((n, K), np.int32), np.zeros((n, K))
    for q0 in range(0, n, CHUNK):
        r = c.knn(x, K, query_start=q0, n_queries=min(CHUNK, n - q0))
        ind[q0:q0 + len(r["indices"])], dist[q0:q0 + len(r["indices"])] = r["indices"], r["distances"]
    t2 = time.perf_counter()
    P = c.tsne_affinities(ind, dist, PERPLEXITY)
    t3 = time.perf_counter()
    y0 = (E.legacy_randn(0, n * 2) * 1e-4).reshape(n, 2)
    csr = (P["indptr"], P["indices"], P["values"])
    c.tsne(*csr, y0, n_iters=2)
    t4 = time.perf_counter()
    r = c.tsne(*csr, y0, n_iters=iters)
    t5 = time.perf_counter()
    c.close()
    print("RESULT " + json.dumps(dict(
        n=n, d=d, K=K, iters=iters, normalize_ms=(t1 - t0) * 1e3, knn_ms=(t2 - t1) * 1e3, affinities_ms=(t3 - t2) * 1e3, search_ms=P["search_ms"],
        csr_ms=P["csr_ms"], nnz=P["nnz"], max_steps=P["max_steps"], call_ms=(t5 - t4) * 1e3, loop_ms=r["loop_ms"], repulse_ms=r["repulse_ms"],
        n_chunks=r["n_chunks"], n_groups=r["n_groups"], row_tile=r["row_tile"], cand_tile=r["cand_tile"], kl=r["kl"])))


def child_sklearn(n, d):
    from sklearn.manifold import TSNE

    X = data(n, d)
    t0 = time.perf_counter()
    m = TSNE(n_components=2, perplexity=PERPLEXITY, method="barnes_hut", angle=0.5, max_iter=250, init="random", random_state=0, n_jobs=16).fit(X)
    print("RESULT " + json.dumps(dict(total_s=time.perf_counter() - t0, n_iter=int(m.n_iter_))))      # its kl_divergence_ is not final at 250


def child_numpy(n, d):
    import knn_numpy
    import tsne_numpy as R

    x = R.normalize(data(n, d))
    t0 = time.perf_counter()
    ind, dist, _ = knn_numpy.knn(x, int(3 * PERPLEXITY))
    t1 = time.perf_counter()
    a = R.affinities(ind, dist, PERPLEXITY)
    t2 = time.perf_counter()
    R.run(a["indptr"], a["indices"], a["values"], R.start(0, n, 2), 0, 1, 250, 250)
    t3 = time.perf_counter()
    print("RESULT " + json.dumps(dict(knn_s=t1 - t0, affinities_s=t2 - t1, iteration_s=t3 - t2)))


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
    n = res["n"]
    per_iter = res["loop_ms"] / res["iters"]
    pairs = float(n) * (n - 1)
    rate = pairs / (res["repulse_ms"] * 1e-3)
    print("n=%d d=%d K=%d: normalise %.1f ms | kNN %.1f ms | affinities %.1f ms (search %.2f + CSR %.2f on the device; nnz %d, at most %d steps) | "
          "loop of %d iterations: %.2f ms per iteration (call %.1f ms) | repulsion %.2f ms of it: %.3g pairs at %.3g pairs/s = %.3g f64 op/s, "
          "%.1f %% of the unfused peak | %d chunks, %d slab groups, row tile %d, candidate tile %d | 1000 iterations: %.1f s BY EXTRAPOLATION from "
          "the %d" % (n, res["d"], res["K"], res["normalize_ms"], res["knn_ms"], res["affinities_ms"], res["search_ms"], res["csr_ms"], res["nnz"],
                     res["max_steps"], res["iters"], per_iter, res["call_ms"], res["repulse_ms"], pairs, rate, rate * OPS_PER_PAIR,
                     100.0 * rate * OPS_PER_PAIR / UNFUSED_PEAK, res["n_chunks"], res["n_groups"], res["row_tile"], res["cand_tile"], per_iter,
                     res["iters"]))
    sys.stdout.flush()
    return per_iter


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--pcs", type=int, default=10)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--force-million", action="store_true")
    ap.add_argument("--child-device", type=int, default=0)
    ap.add_argument("--child-sklearn", type=int, default=0)
    ap.add_argument("--child-numpy", type=int, default=0)
    a = ap.parse_args()
    if a.child_device:
        return child_device(a.child_device, a.pcs, a.iters)
    if a.child_sklearn:
        return child_sklearn(a.child_sklearn, a.pcs)
    if a.child_numpy:
        return child_numpy(a.child_numpy, a.pcs)
    common = ["--pcs", str(a.pcs)]
    per_iter = {}
    for n in (10000, 100000):
        res = run_child(["--child-device", str(n), "--iters", str(a.iters)] + common, LIMITS[n])
        if res is None:
            raise SystemExit("n=%d: the device child ran into its limit of %d s: nothing more is started" % (n, LIMITS[n]))
        per_iter[n] = report(res)
    full = 100.0 * per_iter[100000]      # seconds for 1000 iterations at 1 000 000 cells: 100 x the pairs, ms -> s x 1000 cancels
    if full < 600.0 or a.force_million:
        print("  1 000 000 cells: 100 x the iteration at 100 000 predicts %.0f s for 1000 iterations: measured below" % full)
        iters = a.iters
    else:
        iters = 2 if 5 * 100.0 * per_iter[100000] * 1e-3 < 120.0 else 0      # warm-up 2, 2 timed, the cost's gradient: 5 repulsions
        print("  1 000 000 cells: 100 x the iteration at 100 000 predicts %.0f s for 1000 iterations, NOT under ten minutes: the full run is an "
              "EXTRAPOLATION; %s" % (full, "2 iterations are measured below" if iters else "nothing is measured there"))
    if iters:
        res = run_child(["--child-device", "1000000", "--iters", str(iters)] + common, LIMITS[1000000])
        if res is None:
            raise SystemExit("n=1000000: the device child ran into its limit of %d s: nothing more is started" % LIMITS[1000000])
        report(res)
    if a.no_cpu:
        print("  CPU yardsticks: not timed (--no-cpu)")
        return
    sk = run_child(["--child-sklearn", "10000"] + common, CPU_LIMIT)
    print("  scikit-learn TSNE(method='barnes_hut', angle=0.5), a DIFFERENT algorithm, 10 000 cells, 16 threads: " + (
        "not timed (over %d s)" % CPU_LIMIT if sk is None else "%.1f s for %d iterations with its neighbour search = %.1f ms per iteration | "
        "ratio to the device's iteration %.0f" % (sk["total_s"], sk["n_iter"], sk["total_s"] * 1e3 / sk["n_iter"],
                                                   sk["total_s"] * 1e3 / sk["n_iter"] / per_iter[10000])))
    nu = run_child(["--child-numpy", "10000"] + common, CPU_LIMIT)
    print("  numpy restatement (the same algorithm, exact repulsion), 10 000 cells: " + (
        "not timed (over %d s)" % CPU_LIMIT if nu is None else "kNN %.1f s, affinities %.1f s, one iteration %.2f s | ratio to the device's iteration %.0f" % (
            nu["knn_s"], nu["affinities_s"], nu["iteration_s"], nu["iteration_s"] * 1e3 / per_iter[10000])))


if __name__ == "__main__":
    main()
