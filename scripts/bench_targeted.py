"""Time of the targeted-metrics entry points on the device: Counts.feature_metrics (collapse_feature_counts over the molecule
table) on the cfg3 model, and Context.rpu_gmm (fit_enrichments, BOTH_TIED: 5152 EM fits) at n = 5 000 and n = 20 000 genes.
usage (GPU box): python3 scripts/bench_targeted.py [--reads N] [--repeats 7] [--genes 5000,20000]
tallies  the well of scripts/bench_subsample.py: 10 000 cells and 200 000 ambient barcodes per 10^9 reads (--reads 250000000), one
         library; the cells are the barcodes the generator drew as cells.  TWO contexts in one process, one created with
         CRGPU_FM_LDS_FEATURES unset (LDS slices + slab) and one with CRGPU_FM_LDS_FEATURES=0 (u64 atomics in device memory), each
         with its own count of the same reads; after two warm-up calls each, --repeats calls ALTERNATE between the two: the host
         clock around a call that returns the four arrays (minimum, median, maximum).  Both are compared with the streaming
         bound of the table, 12 B per molecule at 5.5 TB/s; the call itself also reads the keys twice more for the segment
         starts (8 B per molecule each).  The four arrays of the two forms are compared for equality.
fit      values = log10 of a seeded two-group mixture (30 % targeted).  TWO contexts, one created with CRGPU_GMM_LDS_VALUES=16384
         (a start's workgroup keeps the values in LDS, up to 128 KB) and one with =0 (the values are read from device memory, i.e.
         from L2), one warm-up each, then --fit-repeats calls ALTERNATING between the two: the host clock around Context.rpu_gmm
         (minimum, median, maximum) and the library's own fit_ms (host clock from the launch of the 5152 fits until they have
         finished; the copies of the results are not in it), the iterations all starts took, and the rate in (value, iteration)
         pairs per second from fit_ms.  The results of the two forms are compared bit for bit."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cellranger_amd import engine as E  # noqa: E402
from cellranger_amd import synth as S  # noqa: E402


def well(c, w, n):
    c.set_whitelist(0, w.wl_packed, length=16)
    c.set_key_layout(w.n_genes, w.umi_len, 1, 0)
    d = dict(cb=c.empty(n, np.uint32), cbq=c.empty((n, 16), np.uint8), fl=c.empty(n, np.uint8), umi=c.empty(n, np.uint32),
             uq=c.empty((n, 12), np.uint8), ft=c.empty(n, np.uint32), idx=c.empty(n, np.uint32))
    c.synth(w, 0, n, cb=d["cb"].ptr, cb_qualn=d["cbq"].ptr, umi=d["umi"].ptr, umi_qualn=d["uq"].ptr, feature=d["ft"].ptr, flags=d["fl"].ptr)
    c.match_and_count(d["cb"], d["fl"], n, d["idx"])
    c.correct(d["cb"], d["cbq"], d["fl"], n, d["idx"])
    counts = c.count_records(c.records(n, w.umi_len, d["idx"], d["umi"], d["uq"], d["ft"], d["fl"]))
    c.synchronize()
    for v in d.values():
        v.free()
    return counts


def stats(t):
    t = np.sort(np.array(t)) * 1e3
    return t[0], t[len(t) // 2], t[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=250_000_000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--fit-repeats", type=int, default=25)
    ap.add_argument("--genes", default="2000,4000,5000,8000,16000,20000")
    a = ap.parse_args()
    n = a.reads
    if n:
        w = S.Workload(n_total=n, seed=S.SEED0 + 3, n_cells=max(1, n // 100_000), n_ambient=max(1, n // 5_000))
        forms = {}
        for name, env in (("lds slices", None), ("device atomics", "0")):
            os.environ.pop("CRGPU_FM_LDS_FEATURES", None)
            if env is not None:
                os.environ["CRGPU_FM_LDS_FEATURES"] = env      # read when the context is created
            c = E.Context(0)
            forms[name] = (c, well(c, w, n))
        os.environ.pop("CRGPU_FM_LDS_FEATURES", None)
        cell_ranks = np.unique(np.searchsorted(np.sort(w.wl_packed), w.wl_packed[w.cell_wl_pos])).astype(np.uint32)
        nm = forms["lds slices"][1].n_molecules
        cells = {k: c.upload(cell_ranks) for k, (c, _) in forms.items()}
        times, outs = {k: [] for k in forms}, {}
        for rep in range(2 + a.repeats):
            for k, (c, counts) in forms.items():      # alternating
                c.synchronize()
                t0 = time.perf_counter()
                outs[k] = counts.feature_metrics(w.n_genes, cells[k])
                if rep >= 2:
                    times[k].append(time.perf_counter() - t0)
        same = all(np.array_equal(outs["lds slices"][f], outs["device atomics"][f]) for f in outs["lds slices"])
        o = outs["lds slices"]
        bound = nm * 12 / 5.5e12 * 1e3
        print("feature_metrics reads=%d molecules=%d cells=%d features=%d | num_umis=%d num_reads=%d in cells %d / %d | hottest feature: %d molecules | "
              "streaming bound of the table (12 B per molecule at 5.5 TB/s) = %.3f ms | the two forms agree: %s"
              % (n, nm, len(cell_ranks), w.n_genes, int(o["num_umis"].sum()), int(o["num_reads"].sum()), int(o["num_umis_cells"].sum()),
                 int(o["num_reads_cells"].sum()), int(o["num_umis"].max()), bound, same), flush=True)
        for k in forms:
            lo, med, hi = stats(times[k])
            print("  %-15s host ms min=%.3f median=%.3f max=%.3f (%d alternating calls) = %.1f x the bound, %.2f G molecules/s"
                  % (k, lo, med, hi, len(times[k]), med / bound, nm / med / 1e6), flush=True)
        for c, counts in forms.values():
            counts.free()
            c.close()
    forms = {}
    for name, env in (("lds", "16384"), ("device memory", "0")):
        os.environ["CRGPU_GMM_LDS_VALUES"] = env      # read when the context is created
        forms[name] = E.Context(0)
    os.environ.pop("CRGPU_GMM_LDS_VALUES", None)
    for ng in [int(x) for x in a.genes.split(",") if x]:
        rng = np.random.default_rng(ng)
        nt = int(0.3 * ng)
        rpu = np.concatenate([rng.normal(2.8, 0.8, nt).clip(1.05), rng.normal(1.6, 0.3, ng - nt).clip(1.0)])
        values, labels = np.log10(rpu), np.concatenate([np.ones(nt, np.uint8), np.zeros(ng - nt, np.uint8)])
        host, fit, res = {k: [] for k in forms}, {k: [] for k in forms}, {}
        for rep in range(1 + a.fit_repeats):
            for k, c in forms.items():      # alternating
                t0 = time.perf_counter()
                r = c.rpu_gmm(values, labels, want_starts=True)
                if rep >= 1:
                    host[k].append(time.perf_counter() - t0)
                    fit[k].append(r["fit_ms"] / 1e3)
                res[k] = r
        r, q = res["lds"], res["device memory"]
        same = r["start_lk"].tobytes() == q["start_lk"].tobytes() and np.array_equal(r["start_iters"], q["start_iters"]) and all(
            np.float64(r[f]).tobytes() == np.float64(q[f]).tobytes() for f in ("log_rpu_threshold", "mu_high", "mu_low", "sd_high", "alpha_high"))
        its = int(r["start_iters"].sum(dtype=np.int64))
        print("rpu_gmm n=%d starts=%d iterations: total %d, max %d | threshold=%.6f winner=%d classes=%s | the two forms agree bit for bit: %s"
              % (ng, r["n_starts"], its, int(r["start_iters"].max()), r["log_rpu_threshold"], r["winner"],
                 [int(r[f]) for f in ("n_targeted_enriched", "n_targeted_not_enriched", "n_offtgt_enriched", "n_offtgt_not_enriched")], same), flush=True)
        for k in forms:
            lo, med, hi = stats(host[k])
            flo, fmed, fhi = stats(fit[k])
            print("  %-14s in_lds=%d host ms min=%.2f median=%.2f max=%.2f | fit_ms min=%.2f median=%.2f max=%.2f (%d alternating calls) | "
                  "%.1f G (value, iteration) pairs/s" % (k, res[k]["in_lds"], lo, med, hi, flo, fmed, fhi, len(host[k]),
                                                         (its + r["n_starts"]) * ng / fmed / 1e6), flush=True)
    for c in forms.values():
        c.close()

main()
