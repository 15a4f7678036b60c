"""Time of MEASURE_PERTURBATIONS on the device (Context.sseq_pairs, SseqPairs.compare per perturbation, ONE SseqPairs.bootstrap for all
(perturbation, target) items, engine.perturbation_ci; csrc/perturbations.h).
usage (GPU box): python3 scripts/bench_perturbations.py [--shapes 10000:100,100000:1000] [--genes 36601] [--entries 3000] [--draws 500] [--repeats 3]
data      the synthetic filtered matrix of scripts/bench_diffexp.py; a shape is cells:perturbations.  The control is a twentieth of the
          cells (at least 1000), every perturbation takes an equal share of nine tenths of the rest, the other cells are in no group.
          Every perturbation has one target, drawn from the 2000 genes with the most counts.
reports   per shape: the plan, the loop of pair calls, the bootstrap call (median of --repeats after a warm-up) with the draws per second
          it comes to (a draw = one resampled cell: (cells of the perturbation + cells of the control) x bootstraps per item), the
          confidence intervals on the host; then the bootstrap call again with the LDS path switched off (lds_cells = 1) and with 1, 4, 16
          and 32 draws a workgroup -- the values tried; the defaults are 16384 cells and 8 draws.  Every variant is asserted equal to the
          default first.  There is no earlier device path to compare against: at the first shape the numpy restatement
          (tests/perturbations_numpy.py) runs a few items on the CPU, is asserted equal, and its time per draw stands beside the
          device's, recorded as what it is: one Python process on the host."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from cellranger_amd import engine as E  # noqa: E402
import bench_diffexp as BD  # noqa: E402
import perturbations_numpy as P  # noqa: E402


def med(v):
    return float(np.median(v))


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return r, (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="10000:100,100000:1000")
    ap.add_argument("--genes", type=int, default=36601)
    ap.add_argument("--entries", type=int, default=3000)
    ap.add_argument("--draws", type=int, default=500)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--cpu-items", type=int, default=3)
    a = ap.parse_args()
    shapes = [tuple(int(v) for v in s.split(":")) for s in a.shapes.split(",")]
    G, B = a.genes, a.draws
    c = E.Context(0)
    wl = 1
    while wl < max(n for n, _ in shapes):
        wl *= 2
    c.set_whitelist(0, np.arange(wl, dtype=np.uint32), length=16)
    for shape_i, (n, n_pert) in enumerate(shapes):
        t0 = time.perf_counter()
        indptr, indices, data, _ = BD.synth(n, G, a.entries)
        m = BD.upload(c, indptr, indices, data)
        rs = np.random.RandomState(9)
        n_control = max(1000, n // 20)
        per = (n - n_control) * 9 // 10 // n_pert
        groups = np.full(n, -1, np.int32)
        cells = rs.permutation(n)
        groups[cells[:n_control]] = n_pert
        for j in range(n_pert):
            groups[cells[n_control + j * per:n_control + (j + 1) * per]] = j
        gene_counts = np.bincount(indices, weights=data, minlength=G)
        targets = rs.choice(np.argsort(gene_counts)[-2000:], n_pert)
        items = [(int(targets[j]), j, n_pert, j) for j in range(n_pert)]
        draws = float(sum(per + n_control for _ in items)) * B
        print("cells=%d perturbations=%d genes=%d: %d entries, control %d cells, %d cells a perturbation, %d items x %d bootstraps = %.3g draws, "
              "made and uploaded in %.1f s" % (n, n_pert, G, len(indices), n_control, per, len(items), B, draws, time.perf_counter() - t0))

        plan, t_plan = timed(lambda: c.sseq_pairs(m, groups, n_groups=n_pert + 1, n_features=G))
        results, t_pairs = timed(lambda: [plan.compare([j], [n_pert], vectors=False) for j in range(n_pert)])
        print("  plan %.1f ms | %d pair calls %.1f ms (%.2f ms each)" % (t_plan, n_pert, t_pairs, t_pairs / n_pert))

        def boot(**kw):
            return plan.bootstrap(items, n_bootstraps=B, seed=7, **kw)

        ref = boot()
        t_def = [timed(boot)[1] for _ in range(a.repeats)]
        print("  bootstrap, defaults (lds_cells 16384, 8 draws a workgroup): %.2f ms = %.3g draws/s" % (med(t_def), draws / med(t_def) * 1e3))
        for kw in (dict(lds_cells=1), dict(draws_per_wg=1), dict(draws_per_wg=4), dict(draws_per_wg=16), dict(draws_per_wg=32), dict(lds_cells=40960)):
            got = boot(**kw)
            assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]), kw
            t = [timed(lambda: boot(**kw))[1] for _ in range(a.repeats)]
            print("  bootstrap, %s: %.2f ms = %.3g draws/s" % (", ".join("%s=%d" % kv for kv in kw.items()), med(t), draws / med(t) * 1e3))
        _, t_ci = timed(lambda: [E.perturbation_ci(ref[0][i], ref[1][i], results[i]["s_a"], results[i]["s_b"]) for i in range(len(items))])
        print("  confidence intervals on the host: %.1f ms for %d items" % (t_ci, len(items)))

        if shape_i == 0 and a.cpu_items:
            import scipy.sparse as sp

            x = sp.csc_matrix((data, indices, indptr), shape=(G, n)).tocsr()
            t0 = time.perf_counter()
            for g, ka, kb, stream in items[:a.cpu_items]:
                row = np.asarray(x[g].todense()).ravel()
                for z, k in ((0, ka), (1, kb)):
                    want = P.bootstrap_sums(row[np.flatnonzero(groups == k)], 7, stream, z, B)
                    assert np.array_equal(want, ref[z][stream]), (g, k)
            t_cpu = (time.perf_counter() - t0) * 1e3
            d_cpu = float(a.cpu_items * (per + n_control)) * B
            print("  numpy restatement on the CPU, %d items (equal to the device): %.1f ms = %.3g draws/s; the device call is %.0f times that rate" % (
                a.cpu_items, t_cpu, d_cpu / t_cpu * 1e3, (draws / med(t_def)) / (d_cpu / t_cpu)))
        plan.free()
        m.free() if hasattr(m, "free") else None


if __name__ == "__main__":
    main()
