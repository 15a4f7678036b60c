"""Time of the multi-genome analysis on the device (Context.multigenome) beside its numpy restatement on this box's CPU.
usage (GPU box): python3 scripts/bench_multigenome.py [--n 10000,100000] [--bootstraps 1000] [--repeats R] [--no-numpy]
Per n (filtered barcodes of the tests' seeded species mixture: 60 % genome0 cells, 35 % genome1, 5 % doublets) one line with
  call        milliseconds per call: host clock around a call that returns after the device has finished; the two count
              vectors are resident on the device before the clock starts.  Two warm-up calls, then R timed ones (default 50:
              a timed window of half a second at n = 10 000).
  kernels     the context's timing ledger over ONE further call (HIP events around the launches): generator (k_mt19937, one
              workgroup), draws (temper + mask + reject + histogram: the compaction), scan (the row scans), sample
              (k_mg_sample, one workgroup per sample: thresholds, fallback, classes), sorts (the passes of the three radix
              sorts only: k_mg_keys, k_mg_seg_keys, k_mg_places and k_mg_sum_places around them are outside the ledger and
              show only in the call's time).  The ledger's slots are fixed: these are its synth, keys, scan, matrix and
              dedup entries.
  words       raw 32-bit words the generator produced, the expected B * n * (mask + 1) / n, and generator ms / words
and the seconds of tests/multigenome_numpy.py (what the reference runs) for the same call, with whether every per-sample class
count, threshold and branch equals the device's.
Only Context.multigenome is timed: genome_totals and the two column_sums that multigenome_from_matrix runs before it are not."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from cellranger_amd import engine as E  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="10000,100000")
    ap.add_argument("--bootstraps", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--no-numpy", action="store_true")
    a = ap.parse_args()
    import multigenome_numpy as R

    c = E.Context(0)
    B = a.bootstraps
    for n in [int(x) for x in a.n.split(",")]:
        c0, c1 = R.mixture(n, n)
        d0, d1 = c.upload(c0.astype(np.uint32)), c.upload(c1.astype(np.uint32))
        ms, g = [], None
        for rep in range(2 + a.repeats):
            t0 = time.perf_counter()
            g = c.multigenome(d0, d1, B)
            if rep >= 2:
                ms.append((time.perf_counter() - t0) * 1e3)
        ms.sort()
        c.timing(True)
        c.timing_reset()
        c.multigenome(d0, d1, B)
        ledger = c.timing_get()
        c.timing(False)
        by = {k: v[0] for k, v in ledger.items()}
        mask = 1
        while mask < n - 1:
            mask = mask * 2 + 1
        words, expect = g.res["generator_words"], B * (mask + 1)
        line = ("multigenome n=%d bootstraps=%d observed=%s inferred=%d | call ms min=%.2f median=%.2f max=%.2f (%d calls) | kernels ms generator=%.2f "
                "draws=%.2f scan=%.2f sample=%.2f sorts=%.2f | words=%d (expected %d) %.2f Gword/s, generator %.0f %% of the call" % (
                    n, B, g.observed, g.summary["inferred_multiplets"], ms[0], ms[len(ms) // 2], ms[-1], len(ms), by["synth"], by["keys"], by["scan"],
                    by["matrix"], by["dedup"], words, expect, words / max(by["synth"], 1e-9) / 1e6,
                    100 * by["synth"] / ms[0]))
        if not a.no_numpy:
            t0 = time.perf_counter()
            ref = R.run(c0, c1, B)
            t1 = time.perf_counter()
            same = (np.array_equal(ref["boot_counts"], g.boot_counts) and np.array_equal(ref["boot_branch"], g.boot_branch)
                    and np.array_equal(ref["boot_thresholds"].view(np.uint64), g.boot_thresholds.view(np.uint64))
                    and np.array_equal(ref["call"], g.call) and ref["inferred_multiplets"] == g.summary["inferred_multiplets"])
            line += " | numpy s=%.3f (%.2f ms per sample; x%.1f of the device; same result: %s)" % (
                t1 - t0, (t1 - t0) * 1e3 / B, (t1 - t0) * 1e3 / ms[0], same)
        print(line, flush=True)
    c.close()


if __name__ == "__main__":
    main()
