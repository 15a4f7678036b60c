"""Time of RUN_PCA on the device (engine.run_pca) and its split, against the same irlb statements through scipy on the same box.
usage (GPU box): python3 scripts/bench_pca.py [--repeats 3] [--no-scipy] [--only NAME]
data     seeded: 36 601 features, 3 000 entries per cell (ascending features from random gaps of 1 .. 21), three groups of cells whose
         counts are raised on a block of features each; 10 components, every feature above the threshold used (the stage's default).
         Workloads: 10 000 and 100 000 cells.
figure   every workload is measured by a child process of its own with its own time limit (a child that fails or runs into its limit
         ends the script: nothing more is started on the device).  One warm-up call, then --repeats calls; the host clock around the call
         (minimum, median, maximum) and, from the call with the median time, the library's own split into preparation (thresholding,
         dispersion, the PCA matrix in both orders), Lanczos and projection (the full matrix prepared and projected), with mprod.  The time
         per product pair is the Lanczos time over mprod / 2 -- it CONTAINS the dots, the updates and the two scalar reads of a step -- set
         against the streaming bound of the entries: 12 B per entry and direction (an f64 value and a u32 index) at 6.3 TB/s.
scipy    irlb as tests/pca_numpy.py restates it statement by statement (the reference's irlb.py is not on a GPU box), on a scipy CSR matrix
         with the device's own centre, on the SMALLEST workload, within the 16 CPUs a job gets.
What binds the two products is not measured here: no counters are taken."""
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

G, PER_CELL, COMPONENTS = 36601, 3000, 10
WORKLOADS = {"10000": 10000, "100000": 100000}
LIMITS = {"10000": 300, "100000": 900}       # seconds per child
SCIPY_LIMIT = 400
STREAM_BW = 6.3e12


def triplets(n_cells, chunk=5000):
    """-> (barcode, feature, count) u32 arrays, sorted by (barcode, feature)"""
    rs = np.random.RandomState(31)
    fts, cts = [], []
    for lo in range(0, n_cells, chunk):
        n = min(chunk, n_cells - lo)
        ft = rs.randint(1, 22, size=(n, PER_CELL)).cumsum(axis=1)      # at most 63 000 / 2: inside the features with room to spare
        assert ft.max() < G
        group = (np.arange(lo, lo + n) % 3)[:, None]
        ct = 1 + (rs.random_sample((n, PER_CELL)) < 0.25) + 3 * ((ft // 4000) == group) * (rs.random_sample((n, PER_CELL)) < 0.5)
        fts.append(ft.astype(np.uint32).ravel())
        cts.append(ct.astype(np.uint32).ravel())
    return np.repeat(np.arange(n_cells, dtype=np.uint32), PER_CELL), np.concatenate(fts), np.concatenate(cts)


def child_device(name, repeats, out_path):
    from cellranger_amd import engine as E

    n = WORKLOADS[name]
    bc, ft, ct = triplets(n)
    c = E.Context(0)
    c.set_whitelist(0, np.arange(max(n, 1024), dtype=np.uint32), length=16)
    seen = np.zeros(c.n_canon, np.uint32)
    seen[:n] = 1
    c.set_counts(0, 0, seen)
    m = c.assemble_matrix_dev(c.upload(bc), c.upload(ft), c.upload(ct), len(bc))
    E.run_pca(c, m, n_components=COMPONENTS, n_features=G)
    runs = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        r = E.run_pca(c, m, n_components=COMPONENTS, n_features=G)
        runs.append(((time.perf_counter() - t0) * 1e3, r))
    runs.sort(key=lambda t: t[0])
    ms, r = runs[len(runs) // 2]
    res = dict(name=name, cells=n, nnz=int(m.nnz), calls=[t for t, _ in runs], fit_ms=r["fit_ms"], prepare_ms=r["prepare_ms"], lanczos_ms=r["lanczos_ms"],
               project_ms=r["project_ms"], it=r["it"], mprod=r["mprod"], m_b=r["m_b"], used=r["n_used_features"], retried=r["retried"],
               d=[float(x) for x in r["d"]], finite=bool(np.isfinite(r["projection"]).all()))
    np.savez(out_path, d=r["d"], features=r["features_selected"], components=r["components"])
    c.close()
    print("RESULT " + json.dumps(res))


def child_scipy(name, dev_path):
    import scipy.sparse as sp

    import pca_numpy as P

    n = WORKLOADS[name]
    bc, ft, ct = triplets(n)
    dev = np.load(dev_path)
    cols = dev["features"]
    t0 = time.perf_counter()
    m = sp.csr_matrix((ct.astype(np.float64), (bc, ft)), shape=(n, G))      # cells x features; every cell and the used features pass the threshold
    m = m[:, cols].tocsr()
    counts = np.asarray(m.sum(axis=1)).ravel()
    m = sp.diags(max(1.0, np.median(counts)) / counts).dot(m).tocsr()
    m.data = np.log2(1 + m.data)
    from sklearn.utils import sparsefuncs

    mean, var = sparsefuncs.mean_variance_axis(m, axis=0)
    var[var == 0.0] = 1.0
    s = np.sqrt(var)
    sparsefuncs.inplace_column_scale(m, 1.0 / s)
    t1 = time.perf_counter()
    d, v, it, mprod = P.irlb(m, COMPONENTS, mean / s, np.random.RandomState(0).randn(len(cols)))
    t2 = time.perf_counter()
    print("RESULT " + json.dumps(dict(prepare_s=t1 - t0, irlb_s=t2 - t1, it=it, mprod=mprod, max_dev_d=float(np.abs(d - dev["d"]).max() / dev["d"].max()),
                                      threads=os.environ.get("OMP_NUM_THREADS", "unset"))))


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
    pairs = res["mprod"] / 2.0
    per_pair_ms = res["lanczos_ms"] / pairs
    bound_ms = 2 * 12.0 * res["nnz"] / STREAM_BW * 1e3
    print("%s cells: %d entries, %d used features | run_pca call %s ms (min / median / max) | preparation %.1f ms, Lanczos %.1f ms, projection %.1f ms "
          "(library total %.1f ms) | it %d, mprod %d, m_b %d, retried %s" % (res["name"], res["nnz"], res["used"], " / ".join("%.1f" % t for t in res["calls"]),
                                                                             res["prepare_ms"], res["lanczos_ms"], res["project_ms"], res["fit_ms"], res["it"],
                                                                             res["mprod"], res["m_b"], res["retried"]))
    print("  Lanczos per product pair (dots, updates and scalar reads included): %.3f ms; streaming bound of the two products, 12 B per entry and "
          "direction at 6.3 TB/s: %.3f ms = %.1f %% of it | d[0:3] %s | projection finite: %s" % (per_pair_ms, bound_ms, 100.0 * bound_ms / per_pair_ms,
                                                                                                 ["%.4f" % x for x in res["d"][:3]], res["finite"]))
    sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-scipy", action="store_true")
    ap.add_argument("--only", default="")
    ap.add_argument("--child-device", default="")
    ap.add_argument("--child-scipy", default="")
    ap.add_argument("--scratch", default="")
    a = ap.parse_args()
    if a.child_device:
        return child_device(a.child_device, a.repeats, a.scratch)
    if a.child_scipy:
        return child_scipy(a.child_scipy, a.scratch)
    import tempfile

    tmp = tempfile.mkdtemp(prefix="bench_pca_")
    first = True
    for name in WORKLOADS:
        if a.only and name != a.only:
            continue
        path = os.path.join(tmp, "dev_%s.npz" % name)
        res = run_child(["--child-device", name, "--scratch", path, "--repeats", str(a.repeats)], LIMITS[name])
        if res is None:
            raise SystemExit("%s: the device child ran into its limit of %d s: nothing more is started" % (name, LIMITS[name]))
        report(res)
        if first and not a.no_scipy:
            sk = run_child(["--child-scipy", name, "--scratch", path], SCIPY_LIMIT)
            if sk is None:
                print("  scipy: not timed (did not end within %d s)" % SCIPY_LIMIT)
            else:
                print("  scipy on this box (OMP_NUM_THREADS %s): normalise, log, centre and scale %.2f s; irlb %.2f s (it %d, mprod %d; device Lanczos %.1f ms: "
                      "ratio %.0f) | its d is %.2g from the device's, relative to d[0]" % (sk["threads"], sk["prepare_s"], sk["irlb_s"], sk["it"], sk["mprod"],
                                                                                           res["lanczos_ms"], sk["irlb_s"] * 1e3 / res["lanczos_ms"], sk["max_dev_d"]))
        first = False
        sys.stdout.flush()


if __name__ == "__main__":
    main()
