"""Time of the JIBES fit on the device (Context.jibes_fit) against the numpy restatement on the same box.
usage (GPU box): python3 scripts/bench_jibes.py [--repeats 7] [--iterations 60] [--cmo-n 50000] [--mg-n 10000] [--numpy-n 5000]
                 rocprofv3 --kernel-trace --stats -d <dir> -- python3 scripts/bench_jibes.py --trace-run     (a run of its own)
wells    seeded synthetic wells drawn from the model itself (the generator of the test fixtures): 12 tags on --cmo-n barcodes with
         n_gems = 95 000 (limited, 456 latent states) and the two-genome shape, 2 tags on --mg-n barcodes (limited, 11 states).
fit      abs_tol = rel_tol = -inf and max_reps = --iterations - 1, so that exactly --iterations EM iterations run whatever the
         likelihood does.  TWO contexts in one process, one created with CRGPU_JIBES_BATCH unset (the default: the host reads the stop
         latch every 8 rounds) and one with CRGPU_JIBES_BATCH=1 (a host read per iteration); one warm-up call each, then --repeats calls
         ALTERNATING between the two: the host clock around Context.jibes_fit (minimum, median, maximum; it includes the upload of
         y, the final pass and the download of the per-barcode outputs) and the library's own fit_ms (first launch until the latch
         was read as set) per iteration.  The results of the two forms are compared bit for bit.
numpy    tests/jibes_numpy.perform_em on the first --numpy-n barcodes of the 12-tag well (and the whole two-genome well) for 5
         iterations, with the device's time for the same input beside it: time per iteration of both.
The profiler is off in all of this; --trace-run does one warm-up and one fit of the 12-tag well and nothing else."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import jibes_numpy as R  # noqa: E402
from cellranger_amd import engine as E  # noqa: E402

NINF = -float("inf")


def well(seed, n, k, n_gems):
    rng = np.random.RandomState(seed)
    est = E.jibes_expected_cells(n, n_gems)
    states, limited, _, mmk, _ = R.latent_state_setup(n, k, n_gems, estimated_cells=est)
    prior = R.log_prior(states, est, n_gems, limited, mmk)
    w = np.exp(prior) / np.exp(prior).sum()
    zi = rng.choice(len(states), n, p=w)
    bg, fg, sd = rng.uniform(0.8, 1.4, k), rng.uniform(0.6, 0.9, k), rng.uniform(0.3, 0.45, k)
    y = np.log10(rng.poisson(10 ** (bg + fg * states[zi] + rng.normal(0, 1, (n, k)) * sd)) + 1.0)
    return dict(y=y, bg=bg + 0.4, fg=np.maximum(fg - 0.4, 0.05), sd=sd * 2, n_gems=n_gems, est=est, states=states, prior=prior)


def fit(c, w, iterations, n=None):
    y = w["y"] if n is None else np.ascontiguousarray(w["y"][:n])
    est = w["est"] if n is None else E.jibes_expected_cells(len(y), w["n_gems"])
    return c.jibes_fit(y, w["bg"], w["fg"], w["sd"], n_gems=w["n_gems"], estimated_cells=est, abs_tol=NINF, rel_tol=NINF, max_reps=iterations - 1)


def stats(t):
    t = np.sort(np.array(t)) * 1e3
    return t[0], t[len(t) // 2], t[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iterations", type=int, default=60)
    ap.add_argument("--cmo-n", type=int, default=50000)
    ap.add_argument("--mg-n", type=int, default=10000)
    ap.add_argument("--numpy-n", type=int, default=5000)
    ap.add_argument("--trace-run", action="store_true")
    a = ap.parse_args()
    wells = [("12 tags", well(1, a.cmo_n, 12, 95000)), ("2 genomes", well(2, a.mg_n, 2, 95000))]
    os.environ.pop("CRGPU_JIBES_BATCH", None)
    c_def = E.Context(0)
    if a.trace_run:
        fit(c_def, wells[0][1], a.iterations)
        r = fit(c_def, wells[0][1], a.iterations)
        print("trace run: n=%d z=%d iterations=%d fit_ms=%.3f" % (a.cmo_n, r["n_states"], r["iterations"], r["fit_ms"]))
        c_def.close()
        return
    os.environ["CRGPU_JIBES_BATCH"] = "1"
    c_one = E.Context(0)
    os.environ.pop("CRGPU_JIBES_BATCH", None)
    forms = (("default batch", c_def), ("CRGPU_JIBES_BATCH=1", c_one))
    for name, w in wells:
        n, k = w["y"].shape
        z = len(w["states"])
        res, wall, inner = {}, {f: [] for f, _ in forms}, {f: [] for f, _ in forms}
        for f, c in forms:
            fit(c, w, a.iterations)      # warm-up: code objects, pool blocks
        for _ in range(a.repeats):
            for f, c in forms:
                t0 = time.perf_counter()
                r = fit(c, w, a.iterations)
                wall[f].append(time.perf_counter() - t0)
                inner[f].append(r["fit_ms"] * 1e-3)
                res[f] = r
        it = res[forms[0][0]]["iterations"]
        same = all(np.asarray(res[forms[0][0]][q]).tobytes() == np.asarray(res[forms[1][0]][q]).tobytes()
                   for q in ("bg", "fg", "sd", "LL", "probs", "assignment", "assignment_prob", "ml_state"))
        print("%s: n=%d k=%d z=%d iterations=%d (limited=%s) | the two forms agree bit for bit: %s" % (name, n, k, z, it, res[forms[0][0]]["k_let_limited"], same))
        for f, _ in forms:
            lo, med, hi = stats(wall[f])
            ilo, imed, ihi = stats(inner[f])
            print("  %-22s call min/median/max %.3f / %.3f / %.3f ms | fit_ms %.3f / %.3f / %.3f ms | per iteration (median fit_ms) %.1f us | "
                  "%.3g (barcode, state, tag) densities per second" % (f, lo, med, hi, ilo, imed, ihi, imed * 1e3 / it, 2.0 * n * z * k * it / (imed * 1e-3)))
    # the restatement on the same box
    for name, w, nn in ((wells[0][0], wells[0][1], min(a.numpy_n, a.cmo_n)), (wells[1][0], wells[1][1], a.mg_n)):
        y = w["y"][:nn]
        est = E.jibes_expected_cells(nn, w["n_gems"])
        states, limited, _, mmk, _ = R.latent_state_setup(nn, y.shape[1], w["n_gems"], estimated_cells=est)
        prior = R.log_prior(states, est, w["n_gems"], limited, mmk)
        t0 = time.perf_counter()
        ref = R.perform_em(y, states, prior, w["bg"], w["fg"], w["sd"], abs_tol=NINF, rel_tol=NINF, max_reps=4)
        t_np = time.perf_counter() - t0
        fit(c_def, w, 5, nn)
        ts = []
        for _ in range(a.repeats):
            r = fit(c_def, w, 5, nn)
            ts.append(r["fit_ms"] * 1e-3)
        d = max(float(np.max(np.abs(r[q] - ref[q]) / np.abs(ref[q]))) for q in ("bg", "fg", "sd"))
        print("numpy restatement, %s, n=%d z=%d, %d iterations: %.1f ms per iteration (6 E steps, 5 M steps in %.2f s) | device, same input: "
              "%.3f ms per iteration (median fit_ms) | ratio %.0f | largest relative difference of the model %.2g"
              % (name, nn, len(states), ref["iterations"], t_np * 1e3 / ref["iterations"], t_np, stats(ts)[1] / r["iterations"],
                 t_np / ref["iterations"] / (stats(ts)[1] * 1e-3 / r["iterations"]), d))
    c_def.close()
    c_one.close()


if __name__ == "__main__":
    main()
