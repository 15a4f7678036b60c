"""Time of the sSeq differential expression on the device (Context.sseq_params, Context.sseq_diffexp, engine.run_differential_expression)
against the numpy restatement on the same box.
usage (GPU box): python3 scripts/bench_diffexp.py [--sizes 10000,100000] [--genes 36601] [--entries 3000] [--no-cpu] [--repeats 2]
data     a synthetic filtered matrix: --genes x cells, about --entries non-zero genes per cell.  A cell belongs to one of 10 latent groups
         (sizes falling from 22 % to 3 %); it draws gene samples from log-normal gene weights, a twentieth of the genes raised or lowered
         per group; an entry's count is the number of times its gene was drawn.  Seeded.
labels   run_kmeans-style labellings for K = 2 .. 10: cluster = 1 + group % K (every cluster has cells): 54 cluster-against-rest comparisons.
reports  per size: the parameters (one call, host clock); then over the nine labellings the sums of the phase times the library reports
         (group sums, exact tests with their terms and terms per second, asymptotic tests, Benjamini-Hochberg), the exact tests per
         kernel class, and the host clock around engine.run_differential_expression (the whole stage, parameters included).
         --repeats calls after one warm-up; the medians are printed.
cpu      the numpy restatement (tests/sseq_numpy.py) on ONE cluster of the K = 2 labelling at the first size, on a seeded sample of 400
         used genes, scaled by the terms (exact tests) and by the tests (asymptotic) to the 54 comparisons: an EXTRAPOLATION, labelled so."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from cellranger_amd import engine as E  # noqa: E402

KS = list(range(2, 11))
GROUP_SHARE = np.array([22, 18, 14, 11, 9, 8, 7, 5, 3, 3], float) / 100.0


def synth(n_cells, n_genes, entries, seed=11, share=GROUP_SHARE):
    """-> (indptr i64[N + 1], indices u32, data u32, groups i32[N]); the rows of a column ascend; share: the sizes of the latent groups"""
    n_groups = len(share)
    rs = np.random.RandomState(seed)
    w = np.exp(rs.normal(0.0, 1.6, n_genes))
    effect = np.ones((n_groups, n_genes))
    for j in range(n_groups):
        sel = rs.choice(n_genes, n_genes // 20, replace=False)
        effect[j, sel] = np.exp(rs.normal(0.0, 1.2, len(sel)))
    cdfs = [np.cumsum(w * effect[j]) for j in range(n_groups)]
    cdfs = [c / c[-1] for c in cdfs]

    def block(j, n, draws):
        g = np.searchsorted(cdfs[j], rs.random_sample((n, draws)), side="right").astype(np.int64).clip(0, n_genes - 1)
        keys = (np.arange(n, dtype=np.int64)[:, None] * n_genes + g).ravel()
        u, cnt = np.unique(keys, return_counts=True)
        return u // n_genes, (u % n_genes).astype(np.uint32), cnt.astype(np.uint32)

    lo, hi = entries, 40 * entries      # the draws per cell that leave about `entries` distinct genes
    while hi - lo > max(1, entries // 100):
        mid = (lo + hi) // 2
        if len(block(0, 16, mid)[0]) / 16.0 < entries:
            lo = mid
        else:
            hi = mid
    draws = hi
    groups = np.repeat(np.arange(n_groups), np.maximum(1, np.round(np.asarray(share) * n_cells).astype(int)))[:n_cells]
    groups = np.concatenate([groups, np.zeros(n_cells - len(groups), int)])
    rs.shuffle(groups)
    per_cell, idx, dat = np.zeros(n_cells, np.int64), [None] * n_cells, [None] * n_cells
    for j in range(n_groups):
        cells = np.flatnonzero(groups == j)
        for s in range(0, len(cells), 512):
            part = cells[s:s + 512]
            c, g, v = block(j, len(part), draws)
            cuts = np.searchsorted(c, np.arange(len(part) + 1))
            for k, cell in enumerate(part):
                idx[cell], dat[cell] = g[cuts[k]:cuts[k + 1]], v[cuts[k]:cuts[k + 1]]
                per_cell[cell] = cuts[k + 1] - cuts[k]
    indptr = np.concatenate([[0], np.cumsum(per_cell)]).astype(np.int64)
    return indptr, np.concatenate(idx), np.concatenate(dat), groups.astype(np.int32)


def upload(c, indptr, indices, data):
    V = len(indptr) - 1
    seen = np.zeros(c.n_canon, np.uint32)
    seen[:V] = 1
    c.set_counts(0, 0, seen)
    bc = np.repeat(np.arange(V, dtype=np.uint32), np.diff(indptr))
    return c.assemble_matrix_dev(c.upload(bc), c.upload(indices), c.upload(data), len(bc))


def median(v):
    return float(np.median(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="10000,100000")
    ap.add_argument("--genes", type=int, default=36601)
    ap.add_argument("--entries", type=int, default=3000)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    sizes = [int(s) for s in a.sizes.split(",")]
    G = a.genes
    c = E.Context(0)
    wl = 1
    while wl < max(sizes):
        wl *= 2
    c.set_whitelist(0, np.arange(wl, dtype=np.uint32), length=16)
    for n_i, n in enumerate(sizes):
        t0 = time.perf_counter()
        indptr, indices, data, groups = synth(n, G, a.entries)
        m = upload(c, indptr, indices, data)
        m.n_features = G
        clusterings = {"kmeans_%d_clusters" % k: (1 + groups % k).astype(np.int32) for k in KS}
        print("n=%d genes=%d: %d entries (%.0f per cell), made and uploaded in %.1f s" % (n, G, len(indices), len(indices) / n, time.perf_counter() - t0))
        t_par, t_stage, phases = [], [], []
        for rep in range(a.repeats + 1):
            t0 = time.perf_counter()
            params = c.sseq_params(m)
            tp = time.perf_counter() - t0
            ph = dict(ms_sums=0.0, ms_exact=0.0, ms_asymptotic=0.0, ms_bh=0.0, n_terms=0, n_short=0, n_wave=0, n_workgroup=0, n_exact=0, n_asymptotic=0, call=0.0)
            for key, lab in clusterings.items():
                t0 = time.perf_counter()
                r = c.sseq_diffexp(m, params, lab)
                ph["call"] += (time.perf_counter() - t0) * 1e3
                for k in ("ms_sums", "ms_exact", "ms_asymptotic", "ms_bh", "n_terms", "n_short", "n_wave", "n_workgroup"):
                    ph[k] += r[k]
                ph["n_exact"] += int(r["n_exact"].sum())
                ph["n_asymptotic"] += int(r["n_asymptotic"].sum())
            info = params.download()
            t0 = time.perf_counter()
            out = E.run_differential_expression(c, m, clusterings)
            ts = time.perf_counter() - t0
            params.free()
            if rep:      # the first round is the warm-up
                t_par.append(tp * 1e3), t_stage.append(ts * 1e3), phases.append(ph)
        assert sum(v.shape[1] for v in out.values()) == 3 * 54
        p = {k: median([q[k] for q in phases]) for k in phases[0]}
        print("  parameters: %.1f ms (%d of %d genes used, zeta_hat %.3f, delta %.4f)" % (median(t_par), info["n_used"], G, info["zeta_hat"], info["delta"]))
        print("  54 comparisons in 9 calls: %.1f ms on the host clock | group sums %.1f ms | exact tests %.1f ms | asymptotic tests %.1f ms | BH %.1f ms" % (
            p["call"], p["ms_sums"], p["ms_exact"], p["ms_asymptotic"], p["ms_bh"]))
        print("  exact tests: %d (%d short, %d wave, %d workgroup) of %.4g terms: %.3g terms/s | asymptotic tests: %d: %.3g tests/s" % (
            p["n_exact"], p["n_short"], p["n_wave"], p["n_workgroup"], p["n_terms"], p["n_terms"] / (p["ms_exact"] * 1e-3),
            p["n_asymptotic"], p["n_asymptotic"] / max(p["ms_asymptotic"] * 1e-3, 1e-9)))
        print("  the whole stage (engine.run_differential_expression, parameters included): %.1f ms" % median(t_stage))
        if n_i == 0 and not a.no_cpu:
            import scipy.sparse as sp

            import sseq_numpy as R

            rs = np.random.RandomState(3)
            csr = sp.csc_matrix((data.astype(np.int64), indices.astype(np.int64), indptr), shape=(G, n)).tocsr()
            lab = clusterings["kmeans_2_clusters"]
            genes = rs.choice(np.flatnonzero(info["use_g"]), 400, replace=False)
            s_a, s_b = float(info["size_factors"][lab == 1].sum()), float(info["size_factors"][lab != 1].sum())
            t_exact = t_asym = 0.0
            terms = n_as = 0
            for g in genes:
                row = np.asarray(csr[g].todense()).ravel()
                xa, xb = int(row[lab == 1].sum()), int(row[lab != 1].sum())
                t0 = time.perf_counter()
                if xa > R.BIG_COUNT and xb > R.BIG_COUNT:
                    R.asymptotic_p(xa, xb, s_a, s_b, info["mean_g"][g], info["phi_g"][g])
                    t_asym += time.perf_counter() - t0
                    n_as += 1
                else:
                    R.exact_p(xa, xb, s_a, s_b, info["mean_g"][g], info["phi_g"][g])
                    t_exact += time.perf_counter() - t0
                    terms += xa + xb + 1
            cpu_terms = terms / max(t_exact, 1e-9)
            est = p["n_terms"] / cpu_terms + (p["n_asymptotic"] * t_asym / n_as if n_as else 0.0)
            print("  numpy restatement, one thread, %d sampled genes of one cluster: %.3g terms/s, %.2g s per asymptotic test | EXTRAPOLATED to the 54 "
                  "comparisons: %.1f s for the tests alone | ratio to the device's test phases %.0f" % (
                      len(genes), cpu_terms, t_asym / n_as if n_as else float("nan"), est, est * 1e3 / (p["ms_exact"] + p["ms_asymptotic"])))
        m.free()
    c.close()


if __name__ == "__main__":
    main()
