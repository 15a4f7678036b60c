"""Time of RUN_UMAP on the device (engine.run_umap's phases: Context.knn, Context.umap_graph, Context.umap_epochs) against the numpy
restatement on the same box.
usage (GPU box): python3 scripts/bench_umap.py [--epochs 20] [--pcs 10] [--sizes 10000,100000,1000000] [--no-cpu] [--out profiles/umap_throughput.txt]
data     seeded Gaussian blobs (12 of them, sd 3 around centres of sd 4), f64, --pcs columns, n_neighbors 30 (k = 29), the metric
         correlation, 2 output dimensions, the stage's n_epochs (500 up to 10 000 cells, else 200) for the schedule and the prune.
figure   every size is measured by a child process of its own with its own time limit (a child that fails or runs into its limit ends
         the script: nothing more is started on the device).  After a warm-up of each call, the MEDIAN OF 3 calls by the host clock: the
         neighbour search in calls of 15 000 rows (above 100 000 cells ONE search, without a warm-up), the graph (search_ms and csr_ms
         are its device times), Context.umap_epochs for the epochs 50 .. 50 + --epochs (the state of the epochs before them comes from
         one call): call time, loop_ms (events around the loop) / epochs = time per epoch, edges (active entries) and negative samples
         per second over loop_ms.
bound    the bytes an epoch must stream whatever the kernel does: every entry's epoch_of_next_sample (8); per active entry its
         value, index and negative state and both states written back (8 + 4 + 8 + 8 + 8); per row two indptr words, Y read and Y'
         written, the two counters read and written (16 + 16 dims + 32).  The gathers of Y (1 + n_neg rows per active entry) are
         left out: Y is 16 MB at a million cells and stays in the caches.  Over 6.3 TB/s, the copy rate the part reaches.  All of the
         stage's epochs are n_epochs times the epoch measured, BY EXTRAPOLATION.
cpu      one epoch (epoch 50) of the numpy restatement tests/umap_numpy.py on the device's graph and state at 10 000 cells, in a child
         with a time limit.
What binds the epoch kernel is not measured here: no counters are taken."""
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
N_NEIGHBORS = 30
FIRST = 50
COPY_RATE = 6.3e12
LIMITS = {10000: 150, 100000: 240, 1000000: 560}       # seconds per child
CPU_LIMIT = 200


def data(n, d):
    rs = np.random.RandomState(7)
    c = rs.normal(0.0, 4.0, (12, d))
    return np.ascontiguousarray(c[rs.randint(12, size=n)] + rs.normal(0.0, 3.0, (n, d)))


def median3(fn):
    fn()
    out = []
    for _ in range(3):
        t0 = time.perf_counter()
        r = fn()
        out.append(((time.perf_counter() - t0) * 1e3, r))
    out.sort(key=lambda p: p[0])
    return out[1]


def device_graph(c, E, X, n_epochs):
    n, k = len(X), N_NEIGHBORS - 1
    rows = np.ascontiguousarray(E.umap_metric_input(X, "correlation")[0])
    ind, dist = np.zeros((n, k), np.int32), np.zeros((n, k))

    def knn():
        for q0 in range(0, n, CHUNK):
            r = c.knn(rows, k, query_start=q0, n_queries=min(CHUNK, n - q0))
            ind[q0:q0 + len(r["indices"])], dist[q0:q0 + len(r["indices"])] = r["indices"], r["distances"]

    if n <= 100000:
        knn_ms, _ = median3(knn)
    else:      # one search, not the median of 3: it takes tens of seconds there
        t0 = time.perf_counter()
        knn()
        knn_ms = (time.perf_counter() - t0) * 1e3
    d = 0.5 * (dist * dist)
    graph_ms, g = median3(lambda: c.umap_graph(ind, d, n_epochs))
    return knn_ms, graph_ms, g


def child_device(n, d, epochs):
    from cellranger_amd import engine as E

    X = data(n, d)
    n_epochs = 500 if n <= 10000 else 200
    c = E.Context(0)
    knn_ms, graph_ms, g = device_graph(c, E, X, n_epochs)
    a, b = E.umap_ab()
    csr = (g["indptr"], g["indices"], g["values"])
    y0 = E.umap_rescale(X[:, :2])
    s = c.umap_epochs(*csr, y0, a, b, first_epoch=0, n_run=FIRST, n_epochs=n_epochs)
    call_ms, r = median3(lambda: c.umap_epochs(*csr, s["y"], a, b, first_epoch=FIRST, n_run=epochs, n_epochs=n_epochs,
                                                epoch_of_next_sample=s["epoch_of_next_sample"],
                                                epoch_of_next_negative_sample=s["epoch_of_next_negative_sample"]))
    c.close()
    print("RESULT " + json.dumps(dict(
        n=n, d=d, k=N_NEIGHBORS - 1, epochs=epochs, n_epochs=n_epochs, knn_ms=knn_ms, graph_ms=graph_ms, search_ms=g["search_ms"], csr_ms=g["csr_ms"],
        nnz=g["nnz"], max_steps=g["max_steps"], call_ms=call_ms, loop_ms=r["loop_ms"], n_active=r["n_active"], n_negative=r["n_negative"],
        wave_row_len=r["wave_row_len"], rows_per_wg=r["rows_per_wg"], longest_row=int(np.diff(g["indptr"]).max()), finite=bool(np.isfinite(r["y"]).all()))))


def child_numpy(n, d):
    import umap_numpy as R
    from cellranger_amd import engine as E

    X = data(n, d)
    c = E.Context(0)
    _, _, g = device_graph(c, E, X, 500)
    a, b = E.umap_ab()
    csr = (g["indptr"], g["indices"], g["values"])
    s = c.umap_epochs(*csr, E.umap_rescale(X[:, :2]), a, b, first_epoch=0, n_run=FIRST, n_epochs=500)
    c.close()
    t0 = time.perf_counter()
    R.epoch(*csr, s["y"], s["epoch_of_next_sample"], s["epoch_of_next_negative_sample"], FIRST, 500, a, b, 0)
    print("RESULT " + json.dumps(dict(epoch_s=time.perf_counter() - t0)))


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


def report(res, out):
    n, e = res["n"], res["epochs"]
    per_epoch = res["loop_ms"] / e
    act, neg = res["n_active"] / float(e), res["n_negative"] / float(e)
    must = 8.0 * res["nnz"] + 36.0 * act + (16.0 + 16.0 * 2 + 32.0) * n
    line = ("n=%d d=%d k=%d: kNN %.1f ms | graph %.1f ms (search %.2f + union, prune, CSR %.2f on the device; nnz %d, longest row %d, at most %d steps) | "
            "%d epochs from epoch %d: %.3f ms per epoch on the device (call %.1f ms with its copies and checks) | per epoch %.3g active edges and %.3g "
            "negative samples: %.3g edges/s, %.3g samples/s | the epoch must stream %.3g bytes = %.4f ms at 6.3 TB/s: the kernel takes %.0f times "
            "that | all %d epochs: %.2f s BY EXTRAPOLATION | wave_row_len %d, %d threads a workgroup | finite %s" % (
                n, res["d"], res["k"], res["knn_ms"], res["graph_ms"], res["search_ms"], res["csr_ms"], res["nnz"], res["longest_row"], res["max_steps"], e,
                FIRST, per_epoch, res["call_ms"], act, neg, act / (per_epoch * 1e-3), neg / (per_epoch * 1e-3), must, must / COPY_RATE * 1e3,
                per_epoch / (must / COPY_RATE * 1e3), res["n_epochs"], per_epoch * res["n_epochs"] * 1e-3, res["wave_row_len"], res["rows_per_wg"],
                res["finite"]))
    print(line)
    out.append(line)
    sys.stdout.flush()
    return per_epoch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=20)
    ap.add_argument("--pcs", type=int, default=10)
    ap.add_argument("--sizes", default="10000,100000,1000000")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "umap_throughput.txt"))
    ap.add_argument("--child-device", type=int, default=0)
    ap.add_argument("--child-numpy", type=int, default=0)
    a = ap.parse_args()
    if a.child_device:
        return child_device(a.child_device, a.pcs, a.epochs)
    if a.child_numpy:
        return child_numpy(a.child_numpy, a.pcs)
    common = ["--pcs", str(a.pcs)]
    lines, per_epoch = ["scripts/bench_umap.py --epochs %d --pcs %d --sizes %s: the median of 3 calls after a warm-up" % (a.epochs, a.pcs, a.sizes)], {}
    for n in [int(s) for s in a.sizes.split(",")]:
        res = run_child(["--child-device", str(n), "--epochs", str(a.epochs)] + common, LIMITS.get(n, 560))
        if res is None:
            raise SystemExit("n=%d: the device child ran into its limit: nothing more is started" % n)
        per_epoch[n] = report(res, lines)
    if a.no_cpu or 10000 not in per_epoch:
        lines.append("  numpy restatement: not timed")
    else:
        nu = run_child(["--child-numpy", "10000"] + common, CPU_LIMIT)
        lines.append("  numpy restatement (the same step, one thread), 10 000 cells, epoch %d: " % FIRST + (
            "not timed (over %d s)" % CPU_LIMIT if nu is None else "%.3f s | ratio to the device's epoch %.0f" % (
                nu["epoch_s"], nu["epoch_s"] * 1e3 / per_epoch[10000])))
    print(lines[-1])
    lines.append("  what binds the epoch kernel: unmeasured (no counters were taken)")
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
