"""Time of the initial cell call on the device (Context.call_cells_ordmag) beside its numpy restatement on this box's CPU.
usage (GPU box): python3 scripts/bench_cell_calling.py [--n 220623,1048576] [--repeats R] [--no-numpy]
Per N (non-zero barcodes; a third more zero columns are interleaved) one line with the milliseconds per call of
  estimate+call   recovered_cells estimated: 200 bootstrap samples
  call            recovered_cells given: 100 samples
  generator       k_mt19937 alone (one workgroup) over the raw words the 200-sample call consumes, with its rate
and the seconds of tests/ordmag_numpy.py (what the reference runs) for the same two calls.  The count vector is the tests'
well profile (log-normal cells over a geometric ambient tail) and is resident on the device before the clock starts; the
clock is the host's around a call that returns after the device has finished.  Two warm-up calls, then R timed ones."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from cellranger_amd import engine as E  # noqa: E402


def profile(n_nonzero, seed=5):
    rng = np.random.RandomState(seed)
    n_cells = max(1, n_nonzero // 50)
    vals = np.concatenate([np.round(rng.lognormal(8.5, 0.6, n_cells)), rng.geometric(0.15, n_nonzero)])[:n_nonzero]
    vals = np.maximum(vals, 1).astype(np.int64)
    rng.shuffle(vals)
    V = n_nonzero + n_nonzero // 3 + 2
    bc = np.zeros(V, np.int64)
    bc[np.sort(rng.choice(V, n_nonzero, replace=False))] = vals
    return bc


def timed(fn, repeats):
    out = []
    for rep in range(2 + repeats):
        t0 = time.perf_counter()
        fn()
        if rep >= 2:
            out.append((time.perf_counter() - t0) * 1e3)
    return sorted(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="220623,1048576")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-numpy", action="store_true")
    a = ap.parse_args()
    c = E.Context(0)
    for n in [int(x) for x in a.n.split(",")]:
        bc = profile(n)
        d = c.upload(bc.astype(np.uint32))
        given = max(60, n // 30)
        last = {}

        def est():
            last["est"] = c.call_cells_ordmag(d)

        def call():
            last["call"] = c.call_cells_ordmag(d, recovered_cells=given)

        t_est, t_call = timed(est, a.repeats), timed(call, a.repeats)
        mask = 1
        while mask < n - 1:
            mask = mask * 2 + 1
        words = int(200 * n * (mask + 1) / n)
        t_gen = sorted(c.mt19937_stream(0, words)[1] for _ in range(3))
        line = ("cell_calling n_nonzero=%d columns=%d recovered=%d called=%d | estimate+call ms min=%.2f median=%.2f | call(given=%d) ms "
                "min=%.2f median=%.2f | generator %d words ms min=%.2f (%.2f Gword/s; %.0f %% of estimate+call)" % (
                    n, len(bc), last["est"].metrics["recovered_cells"], last["est"].n_cells, t_est[0], t_est[len(t_est) // 2], given,
                    t_call[0], t_call[len(t_call) // 2], words, t_gen[0], words / t_gen[0] / 1e6, 100 * t_gen[0] / t_est[0]))
        if not a.no_numpy:
            import ordmag_numpy as R

            t0 = time.perf_counter()
            cols, ref = R.ordmag(bc)
            t1 = time.perf_counter()
            cols2, ref2 = R.ordmag(bc, recovered_cells=given)
            t2 = time.perf_counter()
            same = (np.array_equal(cols, last["est"].cols_host()) and np.array_equal(cols2, last["call"].cols_host())
                    and np.array_equal(ref["top_n_boot"], last["est"].metrics["top_n_boot"]))
            line += " | numpy s estimate+call=%.3f call=%.3f (x%.1f / x%.1f of the device; same result: %s)" % (
                t1 - t0, t2 - t1, (t1 - t0) * 1e3 / t_est[0], (t2 - t1) * 1e3 / t_call[0], same)
        print(line, flush=True)
    c.close()


if __name__ == "__main__":
    main()
