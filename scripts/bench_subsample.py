"""Time of Counts.subsample (SUBSAMPLE_READS' tallies on the device) on the cfg3 model, and of its draw kernels alone.
usage (GPU box): python3 scripts/bench_subsample.py [--reads N] [--tasks 30] [--repeats 7] [--cpu-molecules M]
The well is the one of scripts/bench_probe_counts.py: 10 000 cells and 200 000 ambient barcodes per 10^9 reads (--reads
250000000 gives 88.9 M molecules).  The cells are the barcodes the generator drew as cells.  The tasks are the depths
crgpu_subsample_plan gives for that well (raw_rpc, conf_mapped_barcoded_filtered_bc_rpc, raw_reads and
raw_barcoded_filtered_bc_rpc, in that order), the first --tasks of them.
GPU      --repeats calls after two warm-up calls: the host clock around a call that returns after the device has finished
         (minimum, median, maximum) and the milliseconds of the draw kernels (crgpu_subsample_result.draw_ms) of the median call.
bound    the streaming bound of the call from its own bytes at 5.5 TB/s: per batch 12 B per molecule read by the draw, 4 B per
         molecule and task written by it, and 12 B per molecule and task read by the tally.
CPU      the numpy restatement (tests/subsample_numpy.kept_vectorised + np.add.reduceat per barcode) for ONE task on the first
         --cpu-molecules molecules of the same table, scaled to the table (the work is linear in the reads)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from cellranger_amd import _lib  # noqa: E402
from cellranger_amd import engine as E  # noqa: E402
from cellranger_amd import synth as S  # noqa: E402
import subsample_numpy as R  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=250_000_000)
    ap.add_argument("--tasks", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--cpu-molecules", type=int, default=2_000_000)
    a = ap.parse_args()
    n = a.reads
    w = S.Workload(n_total=n, seed=S.SEED0 + 3, n_cells=max(1, n // 100_000), n_ambient=max(1, n // 5_000))
    c = E.Context(0)
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
    mol = counts.molecules()
    nm, usable = len(mol["bc"]), int(mol["read_count"].sum(dtype=np.int64))
    cell_ranks = np.unique(np.searchsorted(np.sort(w.wl_packed), w.wl_packed[w.cell_wl_pos])).astype(np.uint32)
    in_cells = int(mol["read_count"][np.isin(mol["bc"], cell_ranks)].sum(dtype=np.int64))
    rates, types = [], []
    for stype, ttype, raw in ((_lib.SS_PLAN_RAW, _lib.SS_PER_CELL, n), (_lib.SS_PLAN_MAPPED, _lib.SS_PER_CELL, n),
                              (_lib.SS_PLAN_BULK, _lib.SS_BULK, n), (_lib.SS_PLAN_RAW_CELLS, _lib.SS_CELLS_ONLY, in_cells)):
        _, r = E.subsample_plan(stype, [0], [len(cell_ranks)], [raw], [usable])
        rates += list(r)
        types += [ttype] * len(r)
    rates, types = np.array(rates[: a.tasks]), types[: a.tasks]
    d_cells = c.upload(cell_ranks)
    times, infos = [], []
    for rep in range(2 + a.repeats):   # the device pool settles in two rounds
        c.synchronize()
        t0 = time.perf_counter()
        out = counts.subsample(rates, types, d_cells, n_features=w.n_genes)
        c.synchronize()
        if rep >= 2:
            times.append(time.perf_counter() - t0)
            infos.append(out["info"])
    order = np.argsort(times)
    med = order[len(order) // 2]
    info = infos[med]
    reads_drawn = int(mol["read_count"].sum(dtype=np.int64))
    T, nb = info["n_active_tasks"], info["n_batches"]
    bound_bytes = nb * 12 * nm + T * 4 * nm + T * 12 * nm
    print("subsample reads=%d molecules=%d reads_in_molecules=%d cells=%d groups=%d tasks=%d (active %d, %d batches) lane/wave/workgroup=%d/%d/%d | "
          "host ms min=%.2f median=%.2f max=%.2f (%d calls) | draw kernels ms=%.2f (%.2f G words/s, %.2f G word-task compares/s) | "
          "streaming bound at 5.5 TB/s = %.2f ms (%.1f GB)"
          % (n, nm, reads_drawn, len(cell_ranks), info["n_groups"], len(types), T, nb, info["n_lane"], info["n_wave"], info["n_workgroup"],
             times[order[0]] * 1e3, times[med] * 1e3, times[order[-1]] * 1e3, len(times), info["draw_ms"],
             nb * reads_drawn / info["draw_ms"] / 1e6, T * reads_drawn / info["draw_ms"] / 1e6, bound_bytes / 5.5e12 * 1e3, bound_bytes / 1e9), flush=True)
    print("  median umis per cell by task:", np.median(out["umis_per_bc"][:, 0, :], axis=1).astype(np.int64).tolist(), flush=True)
    # CPU yardstick: one task, a prefix of the table
    m = min(a.cpu_molecules, nm)
    t = int(np.argmax((np.array(types) == _lib.SS_PER_CELL) & (rates[:, 0] > 0)))
    bc, cnt, lib = mol["bc"][:m], mol["read_count"][:m], mol["lib"][:m]
    t0 = time.perf_counter()
    k = R.kept_vectorised(cnt, lib, rates[t])
    t1 = time.perf_counter()
    starts = np.flatnonzero(np.concatenate(([True], bc[1:] != bc[:-1])))
    rp, um = np.add.reduceat(k, starts), np.add.reduceat((k > 0).astype(np.int64), starts)
    t2 = time.perf_counter()
    scale = reads_drawn / max(1, int(cnt.sum(dtype=np.int64)))
    print("  numpy, one task, %d molecules (%d reads): kept %.2f s, reduceat tallies %.3f s -> %.1f s per task for the table, %.1f s for %d tasks "
          "(kept[:8]=%s read_pairs=%d umis=%d)" % (m, int(cnt.sum()), t1 - t0, t2 - t1, (t2 - t0) * scale, (t2 - t0) * scale * T, T,
                                                     k[:8].tolist(), int(rp.sum()), int(um.sum())), flush=True)
    counts.free()
    c.close()


main()
