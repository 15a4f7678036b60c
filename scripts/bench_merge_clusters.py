"""Time of MERGE_CLUSTERS on the device (engine.merge_clusters, Context.sseq_pairs / SseqPairs.compare, Context.cluster_medians,
engine.linkage_complete) with the composed path of the earlier entry points as the yardstick, in the same run.
usage (GPU box): python3 scripts/bench_merge_clusters.py [--sizes 10000,100000] [--genes 36601] [--entries 3000] [--pcs 10] [--repeats 3]
data      the synthetic filtered matrix of scripts/bench_diffexp.py with 12 latent groups of equal share; the projection is a Gaussian
          cloud of unit spread around a seeded centre per group (spread 8); the labels cut every group at random in two: 24 clusters.
reports   per size, as the median of --repeats calls after one warm-up: engine.merge_clusters as a whole with its own split (plan,
          medians, linkage, pair tests); the plan alone; the medians call and the host linkage at the initial 24 clusters; then for
          every pair the loop tested: the pair call on the host clock and its phases (median, row sums, exact tests, asymptotic tests,
          Benjamini-Hochberg) NEXT TO the same pair through select_barcodes_dev + sseq_params + sseq_diffexp, the outputs asserted equal
          byte for byte first.  The row-sum phase is the host clock around the upload of the size factors, the kernel and the download of
          four G-vectors; beside it stands the streaming bound of the kernel, 12 B per entry of the pair's cells at 6.3 TB/s."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from cellranger_amd import engine as E  # noqa: E402
import bench_diffexp as B  # noqa: E402

N_GROUPS = 12
COPY_BYTES_PER_S = 6.3e12
SAME = (("use", "use_g"), ("mean", "mean_g"), ("phi_mm", "phi_mm_g"), ("phi", "phi_g"))
SAME_ROWS = (("sums_a", "sums_in"), ("sums_b", "sums_out"), ("norm_mean_a", "norm_mean_in"), ("norm_mean_b", "norm_mean_out"),
             ("log2_fold_change", "log2_fold_change"), ("p_values", "p_values"), ("adjusted_p_values", "adjusted_p_values"), ("below_median", "below_median"))


def med(v):
    return float(np.median(v))


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return r, (time.perf_counter() - t0) * 1e3


def composed(c, m, G, cols, na):
    """the pair through the earlier entry points -> (parameters, results, ms of select, parameters, tests)"""
    sub, t_sel = timed(lambda: c.select_barcodes_dev(m, cols))
    params, t_par = timed(lambda: c.sseq_params(sub, n_features=G))
    lab = np.array([1] * na + [2] * (len(cols) - na), np.int32)
    o, t_de = timed(lambda: c.sseq_diffexp(sub, params, lab, 2))
    P = params.download()
    params.free()
    sub.free() if hasattr(sub, "free") else None
    return P, o, (t_sel, t_par, t_de)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="10000,100000")
    ap.add_argument("--genes", type=int, default=36601)
    ap.add_argument("--entries", type=int, default=3000)
    ap.add_argument("--pcs", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    sizes = [int(s) for s in a.sizes.split(",")]
    G = a.genes
    c = E.Context(0)
    wl = 1
    while wl < max(sizes):
        wl *= 2
    c.set_whitelist(0, np.arange(wl, dtype=np.uint32), length=16)
    for n in sizes:
        t0 = time.perf_counter()
        indptr, indices, data, truth = B.synth(n, G, a.entries, share=np.full(N_GROUPS, 1.0 / N_GROUPS))
        m = B.upload(c, indptr, indices, data)
        m.n_features = G
        rs = np.random.RandomState(5)
        pca = rs.normal(0.0, 8.0, (N_GROUPS, a.pcs))[truth] + rs.normal(0.0, 1.0, (n, a.pcs))
        labels = 1 + 2 * truth.astype(np.int64) + rs.randint(0, 2, n)
        per_cell = np.diff(indptr)
        print("n=%d genes=%d pcs=%d: %d entries (%.0f per cell), %d clusters of %d to %d cells, made and uploaded in %.1f s" % (
            n, G, a.pcs, len(indices), len(indices) / n, len(np.unique(labels)), np.bincount(labels)[1:].min(), np.bincount(labels)[1:].max(),
            time.perf_counter() - t0))
        del indices, data

        runs = [E.merge_clusters(c, m, pca, labels) for _ in range(a.repeats + 1)][1:]
        first = runs[0]
        assert all(np.array_equal(r["labels"], first["labels"]) for r in runs)
        print("  engine.merge_clusters: %.1f ms | plan %.1f | medians %.1f | linkage %.2f | pair tests %.1f   (%d -> %d clusters, %d tests, %d skipped, "
              "%d merges, %d iterations)" % (med([r["total_ms"] for r in runs]), med([r["plan_ms"] for r in runs]), med([r["medians_ms"] for r in runs]),
                                             med([r["linkage_ms"] for r in runs]), med([r["pairs_ms"] for r in runs]), first["n_clusters_in"],
                                             first["n_clusters_out"], first["n_tests"], first["n_skipped"], first["n_merges"], first["n_iterations"]))
        groups = (labels - 1).astype(np.int32)
        t_plan = []
        for _ in range(a.repeats + 1):
            plan, t = timed(lambda: c.sseq_pairs(m, groups))
            t_plan.append(t)
            plan.free()
        plan = c.sseq_pairs(m, groups)
        print("  plan (Context.sseq_pairs: one key pass, one 64-bit radix sort of %d entries): %.1f ms" % (len(per_cell) and int(per_cell.sum()), med(t_plan[1:])))
        t_med = [timed(lambda: c.cluster_medians(pca, groups))[1] for _ in range(a.repeats + 1)][1:]
        medoids = c.cluster_medians(pca, groups)["medians"]
        t_link = [timed(lambda: E.linkage_complete(medoids))[1] for _ in range(a.repeats + 1)][1:]
        print("  medians of %d clusters x %d PCs: %.2f ms | host linkage: %.3f ms" % (len(medoids), a.pcs, med(t_med), med(t_link)))

        tot_pair, tot_comp = 0.0, 0.0
        for s in first["steps"]:
            if s["skipped"]:
                continue
            ga, gb = s["groups0"], s["groups1"]
            cols = np.concatenate([np.flatnonzero(groups == g) for g in list(ga) + list(gb)])
            na = int(sum(int((groups == g).sum()) for g in ga))
            entries = int(per_cell[cols].sum())
            got = plan.compare(ga, gb)
            P, o, _ = composed(c, m, G, cols, na)
            for k, pk in SAME:      # asserted equal before anything is timed
                assert np.asarray(got[k]).astype(np.asarray(P[pk]).dtype).tobytes() == np.asarray(P[pk]).tobytes(), (ga, gb, k)
            for k, ok in SAME_ROWS:
                assert np.ascontiguousarray(got[k]).tobytes() == np.ascontiguousarray(o[ok][0]).tobytes(), (ga, gb, k)
            assert (got["zeta_hat"], got["s_a"], got["s_b"], got["n_exact"], got["n_asymptotic"], 2 * got["n_terms"]) == (
                P["zeta_hat"], o["s_a"][0], o["s_b"][0], int(o["n_exact"][0]), int(o["n_asymptotic"][0]), o["n_terms"]) and got["n_de"] == s["n_de"]
            tp, ph, tc = [], [], []
            for _ in range(a.repeats):
                r, t = timed(lambda: plan.compare(ga, gb, vectors=False))
                tp.append(t)
                ph.append([r[k] for k in ("ms_median", "ms_sums", "ms_exact", "ms_asymptotic", "ms_bh")])
                tc.append(composed(c, m, G, cols, na)[2])
            ph, tc = np.median(np.array(ph), axis=0), np.median(np.array(tc), axis=0)
            tot_pair += med(tp)
            tot_comp += float(tc.sum())
            print("  pair %s x %s: %d + %d cells, %d entries, n_de %d | pair call %.2f ms (median %.2f, row sums %.2f [streaming bound %.3f], exact %.2f, "
                  "asymptotic %.2f, BH %.2f) | composed %.2f ms (select %.2f, parameters %.2f, tests %.2f) | ratio %.2f" % (
                      ga, gb, na, len(cols) - na, entries, got["n_de"], med(tp), ph[0], ph[1], entries * 12 / COPY_BYTES_PER_S * 1e3, ph[2], ph[3], ph[4],
                      float(tc.sum()), tc[0], tc[1], tc[2], float(tc.sum()) / med(tp)))
        print("  all %d pairs: pair calls %.1f ms, composed path %.1f ms (ratio %.2f; the plan, %.1f ms, is paid once)" % (
            first["n_tests"], tot_pair, tot_comp, tot_comp / tot_pair, med(t_plan[1:])))
        plan.free()
        m.free() if hasattr(m, "free") else None


if __name__ == "__main__":
    main()
