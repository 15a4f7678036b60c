"""Time of the Louvain stage on the device (Context.louvain on Context.knn's neighbour matrix, as engine.run_graph_clustering(louvain=
"device") runs it) against networkx's serial Louvain on the same box.
usage (GPU box): python3 scripts/bench_louvain.py [--pcs 10] [--sizes 10000,100000,1000000] [--no-cpu] [--out profiles/louvain_throughput.txt]
data     seeded Gaussian blobs (12 of them, sd 3 around centres of sd 4), f64, --pcs columns, k by split()'s rule (250 at 10 000
         cells, 370 at 100 000, 490 at 1 000 000), the neighbour search in calls of 15 000 rows.
figure   every size is measured by a child process of its own with its own time limit (a child that fails or runs into its limit ends
         the script: nothing more is started on the device; a size whose child is not started is reported as unmeasured).  After one
         warm-up call, the MEDIAN OF 3 calls of Context.louvain by the host clock; of that call the library's own split (host clock
         between reads that wait for the device): union_ms (upload, the union and the degrees), rounds_ms, aggregate_ms (the
         renumbering and the next level's graph), their shares of fit_ms; the rounds, nodes and communities of every level; the time
         per round at level 0 = level_ms[0] / (rounds[0] + 1): the level runs one round more than it counts (the one that is
         discarded), and up to batch - 1 latched launches that do nothing.
bound    a round must at least read the CSR once: 8 bytes per entry (index and weight) and 8 per node (indptr), over 6.3 TB/s, the
         copy rate the part reaches.  edges per second = entries of the level-0 graph * rounds run / level_ms[0].
cpu      networkx.community.louvain_communities (seed 0) on the union graph at 10 000 cells, graph construction excluded, in a child
         with a time limit.  It is the serial algorithm in a seeded random visiting order: a DIFFERENT visiting order, so the partitions
         differ; Q of both is printed.
What binds the round is not measured here: no counters are taken."""
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
COPY_RATE = 6.3e12
LIMITS = {10000: 150, 100000: 300, 1000000: 560}       # seconds per child
CPU_LIMIT = 400


def data(n, d):
    rs = np.random.RandomState(7)
    c = rs.normal(0.0, 4.0, (12, d))
    return np.ascontiguousarray(c[rs.randint(12, size=n)] + rs.normal(0.0, 3.0, (n, d)))


def neighbours(c, E, X):
    n = len(X)
    k = E.graphclust_num_neighbors(n)
    srt = np.zeros((n, k), np.int32)
    t0 = time.perf_counter()
    for q0 in range(0, n, CHUNK):
        r = c.knn(X, k, query_start=q0, n_queries=min(CHUNK, n - q0))
        srt[q0:q0 + len(r["sorted_indices"])] = r["sorted_indices"]
    return k, np.arange(n + 1, dtype=np.int64) * k, srt.reshape(-1), (time.perf_counter() - t0) * 1e3


def child_device(n, d):
    from cellranger_amd import engine as E

    X = data(n, d)
    c = E.Context(0)
    k, indptr, indices, knn_ms = neighbours(c, E, X)
    c.louvain(indptr, indices)
    runs = []
    for _ in range(3):
        t0 = time.perf_counter()
        r = c.louvain(indptr, indices)
        runs.append(((time.perf_counter() - t0) * 1e3, r))
    runs.sort(key=lambda p: p[0])
    call_ms, r = runs[1]
    c.close()
    M = float(r["M"])
    print("RESULT " + json.dumps(dict(
        n=n, d=d, k=k, knn_ms=knn_ms, call_ms=call_ms, calls=[p[0] for p in runs], fit_ms=r["fit_ms"], union_ms=r["union_ms"], rounds_ms=r["rounds_ms"],
        aggregate_ms=r["aggregate_ms"], level_ms=r["level_ms"], nodes=r["nodes"], communities=r["communities"], rounds=r["rounds"], nnz=r["nnz"], M=r["M"],
        q=[S / M ** 2 for S in r["S"]], batch=r["batch"], wave_deg_max=r["wave_deg_max"], lds_deg_max=r["lds_deg_max"],
        same=all(np.array_equal(p[1]["final"], r["final"]) and p[1]["S"] == r["S"] for p in runs))))


def child_networkx(n, d):
    import louvain_numpy as R
    import networkx as nx
    from cellranger_amd import engine as E

    X = data(n, d)
    c = E.Context(0)
    _, indptr, indices, _ = neighbours(c, E, X)
    c.close()
    graph = R.union(indptr, indices)
    rows = R.csr_rows(graph[0])
    keep = rows < graph[1]
    G = nx.Graph()
    G.add_nodes_from(range(n))
    G.add_edges_from(zip(rows[keep].tolist(), graph[1][keep].tolist()))
    t0 = time.perf_counter()
    parts = nx.community.louvain_communities(G, seed=0)
    s = time.perf_counter() - t0
    print("RESULT " + json.dumps(dict(seconds=s, communities=len(parts), q=nx.community.modularity(G, parts), version=nx.__version__)))


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
    n, nnz = res["n"], res["nnz"]
    run0 = res["rounds"][0] + 1
    per_round = res["level_ms"][0] / run0
    must = 8.0 * nnz + 8.0 * n
    fit = res["fit_ms"]
    line = ("n=%d d=%d k=%d: kNN %.1f ms | Context.louvain %.1f ms per call (3 calls: %s; the same result every time: %s) | union and degrees %.1f ms "
            "(%.0f %%), rounds %.1f ms (%.0f %%), renumbering and aggregation %.1f ms (%.0f %%) of %.1f ms in the library | level-0 graph %d entries, "
            "M %d | per level nodes %s -> communities %s, counted rounds %s, ms %s, Q %s | level 0: %d rounds run in %.2f ms = %.3f ms per round, "
            "%.3g edges/s | a round must stream %.3g bytes = %.4f ms at 6.3 TB/s: a round takes %.0f times that | batch %d, classes up to %d / %d "
            "entries" % (
                n, res["d"], res["k"], res["knn_ms"], res["call_ms"], ", ".join("%.1f" % v for v in res["calls"]), res["same"], res["union_ms"],
                100 * res["union_ms"] / fit, res["rounds_ms"], 100 * res["rounds_ms"] / fit, res["aggregate_ms"], 100 * res["aggregate_ms"] / fit, fit, nnz,
                res["M"], res["nodes"], res["communities"], res["rounds"], ["%.2f" % v for v in res["level_ms"]], ["%.4f" % v for v in res["q"]], run0,
                res["level_ms"][0], per_round, nnz * run0 / (res["level_ms"][0] * 1e-3), must, must / COPY_RATE * 1e3, per_round / (must / COPY_RATE * 1e3),
                res["batch"], res["wave_deg_max"], res["lds_deg_max"]))
    print(line)
    out.append(line)
    sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pcs", type=int, default=10)
    ap.add_argument("--sizes", default="10000,100000,1000000")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "louvain_throughput.txt"))
    ap.add_argument("--child-device", type=int, default=0)
    ap.add_argument("--child-networkx", type=int, default=0)
    a = ap.parse_args()
    if a.child_device:
        return child_device(a.child_device, a.pcs)
    if a.child_networkx:
        return child_networkx(a.child_networkx, a.pcs)
    common = ["--pcs", str(a.pcs)]
    sizes = [int(s) for s in a.sizes.split(",")]
    lines, device = ["scripts/bench_louvain.py --pcs %d --sizes %s: the median of 3 calls after a warm-up" % (a.pcs, a.sizes)], {}
    for n in sizes:
        res = run_child(["--child-device", str(n)] + common, LIMITS.get(n, 560))
        if res is None:
            raise SystemExit("n=%d: the device child ran into its limit: nothing more is started" % n)
        device[n] = res
        report(res, lines)
    for n in (10000, 100000, 1000000):
        if n not in sizes:
            lines.append("n=%d: not run: UNMEASURED" % n)
    try:
        import networkx  # noqa: F401
        have_nx = True
    except ImportError:
        have_nx = False
    if a.no_cpu or 10000 not in device or not have_nx:
        lines.append("  networkx's serial Louvain: not timed%s" % ("" if have_nx else " (networkx is not installed on this box): UNMEASURED"))
    else:
        nu = run_child(["--child-networkx", "10000"] + common, CPU_LIMIT)
        lines.append("  networkx %s louvain_communities (serial, a seeded random visiting order: a different order, other partitions), 10 000 cells, seed 0: " % (
            nu["version"] if nu else "") + ("not timed (over %d s)" % CPU_LIMIT if nu is None else "%.1f s, %d communities, Q %.4f | the device call is %.0f "
                                            "times faster, its final Q %.4f" % (nu["seconds"], nu["communities"], nu["q"],
                                                                                nu["seconds"] * 1e3 / device[10000]["call_ms"], device[10000]["q"][-1])))
    print(lines[-1])
    lines.append("  what binds the round (bytes or table work): unmeasured (no counters were taken); see DESIGN.md section 4 for the inference")
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
