"""Time of Counts.normalize_depth (aggr's NORMALIZE_DEPTH for one GEM well on the device) on the cfg3 model, and of its draw and
tally steps alone.
usage (GPU box): python3 scripts/bench_normalize_depth.py [--reads N] [--repeats 7] [--cpu-molecules M]
The well is the one of scripts/bench_subsample.py with its reads spread over two libraries: 10 000 cells and 200 000 ambient
barcodes per 10^9 reads (--reads 250000000).  The cells are the barcodes the generator drew as cells; the features are two
classes (the lower and the upper half) and every cell is a cell of both.  frac_reads_kept = (0.5, 0.25).
GPU      --repeats calls after two warm-up calls (the first one makes the position map of a two-library table on the host, once
         per counts): the host clock around a call that returns the matrix and the sums (minimum, median, maximum) and the
         milliseconds of the draw kernels and of the tally (crgpu_normalize_depth_result.draw_ms / tally_ms) of the median call.
bound    the streaming bound of the call from its own bytes at 5.5 TB/s: per molecule 12 B read by the prep, 12 B read and 4 B
         written by the draw, 20 B read by the sums (key, reads, kept, position), 4 B and then 12 B read by the two passes of the
         survivor compaction; per survivor 8 B written by it and 16 B read by the two passes of the head compaction; per triplet
         12 B written by it, 8 B for the counts, 12 B read and 8 B written by the assembly.
CPU      the numpy restatement (tests/subsample_numpy.kept_vectorised, then np.unique with counts on the (barcode, feature) pairs
         of the survivors) on the first --cpu-molecules molecules of the same table, scaled to the table (linear in the reads)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from cellranger_amd import engine as E  # noqa: E402
from cellranger_amd import synth as S  # noqa: E402
import subsample_numpy as R  # noqa: E402

FRAC = (0.5, 0.25)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=250_000_000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--cpu-molecules", type=int, default=2_000_000)
    a = ap.parse_args()
    n = a.reads
    w = S.Workload(n_total=n, seed=S.SEED0 + 3, n_cells=max(1, n // 100_000), n_ambient=max(1, n // 5_000), n_libs=2)
    c = E.Context(0)
    for lib in range(2):
        c.set_whitelist(lib, w.wl_packed, length=16)
    c.set_key_layout(w.n_genes, w.umi_len, 2, 0)
    d = dict(cb=c.empty(n, np.uint32), cbq=c.empty((n, 16), np.uint8), fl=c.empty(n, np.uint8), umi=c.empty(n, np.uint32),
             uq=c.empty((n, 12), np.uint8), ft=c.empty(n, np.uint32), idx=c.empty(n, np.uint32))
    c.synth(w, 0, n, cb=d["cb"].ptr, cb_qualn=d["cbq"].ptr, umi=d["umi"].ptr, umi_qualn=d["uq"].ptr, feature=d["ft"].ptr, flags=d["fl"].ptr)
    c.match_and_count(d["cb"], d["fl"], n, d["idx"])
    c.correct(d["cb"], d["cbq"], d["fl"], n, d["idx"])
    counts = c.count_records(c.records(n, w.umi_len, d["idx"], d["umi"], d["uq"], d["ft"], d["fl"]))
    c.synchronize()
    for v in d.values():
        v.free()
    mol = counts.molecules()
    nm, reads = len(mol["bc"]), int(mol["read_count"].sum(dtype=np.int64))
    print("table: reads=%d molecules=%d reads_in_molecules=%d per library %s" % (n, nm, reads, np.bincount(mol["lib"], minlength=2).tolist()),
          flush=True)
    cell_ranks = np.unique(np.searchsorted(np.sort(w.wl_packed), w.wl_packed[w.cell_wl_pos])).astype(np.uint32)
    fclass = (np.arange(w.n_genes) >= w.n_genes // 2).astype(np.uint8)
    d_cells = c.upload(cell_ranks)
    times, infos = [], []
    for rep in range(2 + a.repeats):
        c.synchronize()
        t0 = time.perf_counter()
        out = counts.normalize_depth(FRAC, cell_ranks=d_cells, feature_class=fclass, n_classes=2)
        c.synchronize()
        if rep == 0:
            print("first call (with the position map): %.2f s" % (time.perf_counter() - t0), flush=True)
        if rep >= 2:
            times.append(time.perf_counter() - t0)
            infos.append(out.result)
        if rep < 1 + a.repeats:
            out.matrix.free()
    order = np.argsort(times)
    med = order[len(order) // 2]
    info = infos[med]
    ns, nt = info["n_kept_molecules"], info["n_triplets"]
    bound_bytes = nm * (12 + 16 + 20 + 4 + 12) + ns * (8 + 16) + nt * (12 + 8 + 12 + 8)
    print("normalize_depth reads=%d molecules=%d cells=%d frac=%s lane/wave/workgroup=%d/%d/%d kept molecules=%d triplets=%d columns=%d | "
          "host ms min=%.2f median=%.2f max=%.2f (%d calls) | draw kernels ms=%.2f (%.2f G words/s) | tally ms=%.2f (%.2f G molecules/s) | "
          "streaming bound at 5.5 TB/s = %.2f ms (%.2f GB)"
          % (n, nm, len(cell_ranks), list(FRAC), info["n_lane"], info["n_wave"], info["n_workgroup"], ns, nt, out.matrix.n_barcodes,
             times[order[0]] * 1e3, times[med] * 1e3, times[order[-1]] * 1e3, len(times), info["draw_ms"], reads / info["draw_ms"] / 1e6,
             info["tally_ms"], nm / info["tally_ms"] / 1e6, bound_bytes / 5.5e12 * 1e3, bound_bytes / 1e9), flush=True)
    print("  raw_mapped_reads=%s flt_mapped_reads=%s kept_reads_per_lib=%s of %s" % (out.raw_mapped_reads.tolist(), out.flt_mapped_reads.tolist(),
                                                                                  out.kept_reads_per_lib.tolist(), out.reads_per_lib.tolist()), flush=True)
    # CPU yardstick: a prefix of the table
    m = min(a.cpu_molecules, nm)
    bc, ft, cnt, lib = mol["bc"][:m].astype(np.int64), mol["feature"][:m].astype(np.int64), mol["read_count"][:m], mol["lib"][:m]
    t0 = time.perf_counter()
    k = R.kept_vectorised(cnt, lib, FRAC, seed=0)
    t1 = time.perf_counter()
    surv = k > 0
    pairs, umis = np.unique(bc[surv] * w.n_genes + ft[surv], return_counts=True)
    t2 = time.perf_counter()
    scale = reads / max(1, int(cnt.sum(dtype=np.int64)))
    print("  numpy, %d molecules (%d reads): kept %.2f s, np.unique on the pairs %.3f s -> %.1f s for the table "
          "(kept[:8]=%s triplets=%d umis=%d)" % (m, int(cnt.sum()), t1 - t0, t2 - t1, (t2 - t0) * scale, k[:8].tolist(), len(pairs), int(umis.sum())),
          flush=True)
    out.matrix.free()
    counts.free()
    c.close()


main()
