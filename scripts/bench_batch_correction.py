"""Time of CORRECT_CHEMISTRY_BATCH on the device (engine.correct_chemistry_batch) and its split, against the reference's two hot functions
through scikit-learn on the same box.
usage (GPU box): python3 scripts/bench_batch_correction.py [--repeats 3] [--no-sklearn] [--only NAME]
data     seeded: 8 cluster centres (sd 1 per dimension) shared by the batches, a per-batch shift of sd 0.05 (0.01 at d = 100), noise of sd
         0.1 per dimension at d = 10 and 0.03 at d = 100; the rows of a batch are contiguous; knn = 10, alpha = 0.1, sigma = 150.
         Workloads: two batches of 20 000 cells at d = 10 and at d = 100; four batches of 32 000 at d = 100 (the stage's cap of 128 000).
figure   every workload is measured by a child process of its own with its own time limit (a child that fails or runs into its limit
         ends the script: nothing more is started on the device).  One warm-up call, then --repeats calls; the host clock around the
         call (minimum, median, maximum) and, from the call with the median time: the cross queries (the sum of their calls' host time),
         the mutual pairs and the schedule (host), the two scores, and of Context.batch_correct the upload, the download and per step
         the device time of gather, accumulate, finish and apply from events around the kernels.  (row, pair) evaluations per second =
         the sum over the steps of n_cur * n_mnn over the accumulate time.  The accumulate kernel's f64 rate counts 5 d operations per
         evaluation (3 d for d2, 2 d for the weighted sum; the exp is reported as exps per second beside it) against 39.3e12
         operations per second: half of the part's 78.6 Tflop/s f64 vector peak, since unfused code (-ffp-contract=off) cannot use
         the multiply-add's other half.
sklearn  what find_knn and correction_vector do, on the same box's CPUs within the 16 a job gets, on the SMALLEST workload: BallTree(ref,
         leaf_size = 40).query(cur, 10) in both directions, and rbf_kernel(cur, mnn_cur, gamma = 0.5 sigma), the product of the weights
         with the pair differences (BLAS) and the division, the cur rows in chunks of 2000 to bound the memory (the reference takes
         them all at once).  Figures for the larger workloads are BY EXTRAPOLATION: the small one's times scaled by the queries *
         candidates * d and by the evaluations * d; they are labelled so.
What binds the accumulate kernel is not measured here: no counters are taken."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = {"2x20000_d10": (2, 20000, 10), "2x20000_d100": (2, 20000, 100), "4x32000_d100": (4, 32000, 100)}
LIMITS = {"2x20000_d10": 240, "2x20000_d100": 300, "4x32000_d100": 400}       # seconds per child
SKLEARN_LIMIT = 400
PEAK_UNFUSED = 39.3e12
KNN, SIGMA = 10, 150.0


def data(nb, per, d):
    rs = np.random.RandomState(11)
    centres = rs.normal(size=(8, d))
    noise, shift = (0.1, 0.05) if d <= 10 else (0.03, 0.01)
    rows = [centres[rs.randint(8, size=per)] + rs.normal(size=d) * shift + rs.normal(size=(per, d)) * noise for _ in range(nb)]
    return np.ascontiguousarray(np.concatenate(rows)), np.repeat(np.arange(nb), per)


def child_device(name, repeats, out_path):
    from cellranger_amd import engine as E

    nb, per, d = WORKLOADS[name]
    x, ids = data(nb, per, d)
    c = E.Context(0)
    E.correct_chemistry_batch(c, x, ids)
    runs = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        r = E.correct_chemistry_batch(c, x, ids)
        runs.append(((time.perf_counter() - t0) * 1e3, r))
    runs.sort(key=lambda t: t[0])
    ms, r = runs[len(runs) // 2]
    cr = r["correct"]
    res = dict(name=name, n=len(x), d=d, calls=[t for t, _ in runs], knn_ms=r["knn_ms"], mnn_ms=r["mnn_ms"], score_ms=r["score_ms"],
               correct_ms=cr["fit_ms"], upload_ms=cr["upload_ms"], download_ms=cr["download_ms"], step_ms=cr["step_ms"].tolist(),
               accumulate_ms=cr["accumulate_ms"], evaluations=cr["pairs_evaluated"], chunks=cr["chunks"], pair_tile=cr["pair_tile"], row_tile=cr["row_tile"],
               steps=[(s["n_cur"], s["n_mnn"]) for s in r["steps"]], overlap=[float(v) for v in r["overlap"].values()],
               scores=[r["batch_score_before"], r["batch_score_after"]], finite=bool(np.isfinite(r["aligned"]).all()))
    np.savez(out_path, aligned=r["aligned"][::997], mnn=r["mutual_nn"][(0, 1)])
    c.close()
    print("RESULT " + json.dumps(res))


def child_sklearn(name, dev_path):
    from sklearn.metrics.pairwise import rbf_kernel
    from sklearn.neighbors import BallTree

    nb, per, d = WORKLOADS[name]
    x, _ = data(nb, per, d)
    dev = np.load(dev_path)
    t0 = time.perf_counter()
    nn = {}
    for i, j in ((0, 1), (1, 0)):
        nn[(i, j)] = BallTree(x[j * per:(j + 1) * per], leaf_size=40).query(x[i * per:(i + 1) * per], k=KNN, return_distance=False) + j * per
    t1 = time.perf_counter()
    mnn = dev["mnn"]                                    # the device's mutual pairs: batch 1 moves towards batch 0
    mnn_cur, mnn_ref = x[mnn[:, 1]], x[mnn[:, 0]]
    bias = mnn_ref - mnn_cur
    corr = np.zeros((per, d))
    for lo in range(0, per, 2000):
        w = rbf_kernel(x[per + lo:per + lo + 2000], mnn_cur, gamma=0.5 * SIGMA)
        corr[lo:lo + 2000] = np.dot(w, bias) / np.sum(w, axis=1)[:, None]
    t2 = time.perf_counter()
    aligned = x.copy()
    aligned[per:] += corr
    got, want = aligned[::997], dev["aligned"]
    scale = np.abs(want).max()
    print("RESULT " + json.dumps(dict(knn_s=t1 - t0, corr_s=t2 - t1, n_mnn=len(mnn), max_dev=float(np.nanmax(np.abs(got - want)) / scale),
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
    calls, d = res["calls"], res["d"]
    acc_s = res["accumulate_ms"] * 1e-3
    ev = res["evaluations"]
    print("%s: n=%d d=%d | stage call %s ms (min / median / max) | cross queries %.1f ms, mutual pairs + schedule %.1f ms, scores %.1f ms, "
          "batch_correct %.1f ms (upload %.1f, download %.1f)" % (res["name"], res["n"], d, " / ".join("%.1f" % t for t in calls), res["knn_ms"],
                                                                   res["mnn_ms"], res["score_ms"], res["correct_ms"], res["upload_ms"], res["download_ms"]))
    for s, ((n_cur, n_mnn), ms) in enumerate(zip(res["steps"], res["step_ms"])):
        print("  step %d: %d cur rows x %d pairs | gather %.3f ms, accumulate %.3f ms, finish %.3f ms, apply %.3f ms" % (s, n_cur, n_mnn, ms[0], ms[1], ms[2], ms[3]))
    if acc_s > 0:
        print("  accumulate: %.4g (row, pair) evaluations in %.3f ms = %.3g per second; %.3g f64 operations per second at 5 d per evaluation = "
              "%.1f %% of the unfused f64 vector peak (39.3e12), beside %.3g exps per second | pair tile %d, row tile %d, %d chunks" % (
                  ev, res["accumulate_ms"], ev / acc_s, 5.0 * d * ev / acc_s, 100.0 * 5.0 * d * ev / acc_s / PEAK_UNFUSED, ev / acc_s, res["pair_tile"],
                  res["row_tile"], res["chunks"]))
    print("  overlaps %s | batch score %.4f -> %.4f | aligned finite: %s" % (["%.3f" % v for v in res["overlap"]], res["scores"][0], res["scores"][1], res["finite"]))
    sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-sklearn", action="store_true")
    ap.add_argument("--only", default="")
    ap.add_argument("--child-device", default="")
    ap.add_argument("--child-sklearn", default="")
    ap.add_argument("--scratch", default="")
    a = ap.parse_args()
    if a.child_device:
        return child_device(a.child_device, a.repeats, a.scratch)
    if a.child_sklearn:
        return child_sklearn(a.child_sklearn, a.scratch)
    import tempfile

    tmp = tempfile.mkdtemp(prefix="bench_bc_")
    small = None
    for name in WORKLOADS:
        if a.only and name != a.only:
            continue
        path = os.path.join(tmp, "dev_%s.npz" % name)
        res = run_child(["--child-device", name, "--scratch", path, "--repeats", str(a.repeats)], LIMITS[name])
        if res is None:
            raise SystemExit("%s: the device child ran into its limit of %d s: nothing more is started" % (name, LIMITS[name]))
        report(res)
        nb, per, d = WORKLOADS[name]
        if small is None:
            if a.no_sklearn:
                print("  scikit-learn: not timed (--no-sklearn)")
                continue
            sk = run_child(["--child-sklearn", name, "--scratch", path], SKLEARN_LIMIT)
            if sk is None:
                print("  scikit-learn: not timed (did not end within %d s)" % SKLEARN_LIMIT)
                continue
            small = dict(sk=sk, queries=2.0 * per * per * d, work=float(res["evaluations"]) * d, res=res)
            print("  scikit-learn on this box (OMP_NUM_THREADS %s): BallTree build + query, both directions %.2f s (device cross queries %.1f ms: ratio "
                  "%.0f) | rbf_kernel + dot + division over %d pairs %.2f s (device batch_correct %.1f ms: ratio %.0f) | its aligned rows are %.2g "
                  "from the device's, relative to the largest entry" % (
                      sk["threads"], sk["knn_s"], res["knn_ms"], sk["knn_s"] * 1e3 / res["knn_ms"], sk["n_mnn"], sk["corr_s"], res["correct_ms"],
                      sk["corr_s"] * 1e3 / res["correct_ms"], sk["max_dev"]))
        else:
            knn_s = small["sk"]["knn_s"] * nb * (nb - 1) * per * per * d / small["queries"]
            corr_s = small["sk"]["corr_s"] * res["evaluations"] * d / small["work"]
            print("  scikit-learn BY EXTRAPOLATION from the first workload (not timed): cross queries %.1f s (brute-force scaling; a tree does "
                  "better at low d and worse at high d), corrections %.1f s" % (knn_s, corr_s))
        sys.stdout.flush()


if __name__ == "__main__":
    main()
