"""Time of the multiplexed-Flex calls on the device beside a vectorised numpy restatement on this box's CPU.
usage (GPU box): python3 scripts/bench_rtl_tags.py [--gels 500000] [--columns 4000000] [--cells 128000] [--repeats R] [--no-numpy]
The well is synthetic and seeded: 16 probe barcodes = 16 tags, `gels` gel beads (a canonical space of gels x 16), `columns` raw
columns drawn from it without replacement, a Poisson(3) number of entries per column (at most 12) over 2000 features (the last 10 Antibody
Capture), and about `cells` cells taken from the columns of a random 12 % of the gel beads, so that GEMs with several cells exist.
One line per call:
  rtl_tags            Context.rtl_tags with the feature types (section 1: tags, barcodes per tag, UMIs per type and tag)
  rtl_gem_runs        Context.rtl_gem_runs without the antibody part (section 3: overlaps and GEM occupancy)
  remove_high_occ     Context.remove_high_occupancy_gems at threshold 2 (section 6)
with the median / min / max milliseconds of the timed calls (2 warm-up calls, then at least R = 20 and as many as fill half a
second; host clock around a call that returns after the device has finished and the small tables have been copied back), the
call's streaming bound from its own bytes at 5.5 TB/s,
and the seconds of the vectorised numpy restatement of the same call with whether the results are equal.  Bytes counted:
  rtl_tags            4 V (ranks) + V (tags written) + 8 (V + 1) (indptr) + 8 nnz (indices, data) + V (tags read back by the UMI pass)
  rtl_gem_runs        V (flag memset) + 8 n_cells + n_cells (flag scatter) + 4 V + V + V (ranks, tags, flags; neighbours from L2)
  remove_high_occ     n_cells (8 + 4 + 1) (columns, gathered ranks, keep flags) + 9 n_cells (compaction reads) + 8 kept"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cellranger_amd import engine as E  # noqa: E402

BW = 5.5e12
N_PROBE, N_FEATURES, N_AB = 16, 2000, 10


def timed(fn, repeats):
    """two warm-up calls, then at least `repeats` timed ones and as many as fill half a second"""
    ms, out = [], None
    for _ in range(2):
        t0 = time.perf_counter()
        out = fn()
        warm = time.perf_counter() - t0
    n = max(repeats, int(0.5 / max(warm, 1e-6)) + 1)
    for _ in range(n):
        t0 = time.perf_counter()
        out = fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    ms.sort()
    return out, ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gels", type=int, default=500000)
    ap.add_argument("--columns", type=int, default=4000000)
    ap.add_argument("--cells", type=int, default=128000)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--no-numpy", action="store_true")
    a = ap.parse_args()
    rng = np.random.RandomState(20)
    n_canon = a.gels * N_PROBE
    ranks = np.sort(rng.choice(n_canon, a.columns, replace=False)).astype(np.uint32)
    V = len(ranks)
    per_col = rng.poisson(3.0, V)
    per_col = np.minimum(per_col, 12)
    indptr = np.concatenate([[0], np.cumsum(per_col)]).astype(np.int64)
    nnz = int(indptr[-1])
    # distinct ascending features inside a column: a random start plus a fixed stride (the twelfth entry reaches the Antibody rows)
    start = rng.randint(0, 200, V)
    within = np.arange(nnz) - np.repeat(indptr[:-1], per_col)
    feat = (np.repeat(start, per_col) + within * 163).astype(np.uint32)
    assert feat.max() < N_FEATURES
    data = rng.randint(1, 30, nnz).astype(np.uint32)
    ftype = np.zeros(N_FEATURES, np.uint8)
    ftype[-N_AB:] = 1
    gel = ranks // N_PROBE
    chosen = np.zeros(a.gels, bool)
    chosen[rng.choice(a.gels, int(a.gels * 0.12), replace=False)] = True
    cand = np.flatnonzero(chosen[gel])
    cells = np.sort(rng.choice(cand, min(a.cells, len(cand)), replace=False)).astype(np.uint64)

    c = E.Context(0)
    c.set_barcode_segments(0, [np.arange(a.gels, dtype=np.uint32), np.arange(N_PROBE, dtype=np.uint32)], [16, 8])
    seen = np.zeros(n_canon, np.uint32)
    seen[ranks] = 1
    c.set_counts(0, 0, seen)
    m = c.assemble_matrix_dev(c.upload(np.repeat(ranks, per_col)), c.upload(feat), c.upload(data), nnz)
    assert m.n_barcodes == V and m.nnz == nnz
    call = E.CellCall(c, c.upload(cells), len(cells), {"filtered_bcs": len(cells)}, m)
    top = np.arange(N_PROBE, dtype=np.uint8)
    print("well: %d gel beads x %d probe barcodes, V=%d raw columns, nnz=%d, %d cells in %d GEMs, %d tags" % (
        a.gels, N_PROBE, V, nnz, len(cells), len(np.unique(gel[cells.astype(np.int64)])), N_PROBE), flush=True)

    def line(name, ms, nbytes, np_s, same):
        bound = nbytes / BW * 1e3
        s = "%-16s ms median=%.3f min=%.3f max=%.3f (%d calls) | %.1f MB -> streaming bound %.4f ms at 5.5 TB/s (x%.1f of it)" % (
            name, ms[len(ms) // 2], ms[0], ms[-1], len(ms), nbytes / 1e6, bound, ms[len(ms) // 2] / bound)
        if np_s is not None:
            s += " | numpy s=%.3f (x%.0f of the device; same result: %s)" % (np_s, np_s * 1e3 / ms[len(ms) // 2], same)
        print(s, flush=True)

    # ---- section 1 ----
    tags, ms = timed(lambda: c.rtl_tags(m, top, N_PROBE, ftype, 2), a.repeats)
    np_s = same = None
    if not a.no_numpy:
        t0 = time.perf_counter()
        h_tags = top[ranks % N_PROBE]
        per_tag = np.bincount(h_tags, minlength=N_PROBE)
        key = ftype[feat].astype(np.int64) * N_PROBE + np.repeat(h_tags, per_col)
        umi = np.bincount(key, weights=data.astype(np.float64), minlength=2 * N_PROBE).astype(np.uint64).reshape(2, N_PROBE)   # exact below 2^53
        np_s = time.perf_counter() - t0
        same = (np.array_equal(tags.tags, h_tags) and np.array_equal(tags.barcodes_per_tag, per_tag.astype(np.uint64))
                and np.array_equal(tags.umi_per_tag, umi))
    line("rtl_tags", ms, 4 * V + V + 8 * (V + 1) + 8 * nnz + V, np_s, same)

    # ---- section 3 ----
    runs, ms = timed(lambda: c.rtl_gem_runs(m, tags, call), a.repeats)
    if not a.no_numpy:
        t0 = time.perf_counter()
        ci = cells.astype(np.int64)
        g, t = gel[ci], top[ranks[ci] % N_PROBE]
        ug, first, per_gem = np.unique(g, return_index=True, return_counts=True)
        mask = np.bitwise_or.reduceat(np.uint64(1) << t.astype(np.uint64), first)
        bit = [(mask >> np.uint64(k)) & np.uint64(1) for k in range(N_PROBE)]
        gems = np.array([b.sum() for b in bit], np.uint64)
        common = np.zeros((N_PROBE, N_PROBE), np.uint64)
        for i in range(N_PROBE):
            for j in range(i + 1, N_PROBE):
                common[i, j] = (bit[i] & bit[j]).sum()
        hist = np.bincount(per_gem, minlength=N_PROBE + 1).astype(np.uint64)
        hist[0] = 0
        cpp = np.bincount(ranks[ci] % N_PROBE, minlength=N_PROBE).astype(np.uint64)
        np_s = time.perf_counter() - t0
        same = (np.array_equal(runs.gems_per_tag, gems) and np.array_equal(runs.common, common) and runs.gems_with_cells == len(ug)
                and np.array_equal(runs.cells_per_gem_hist, hist) and np.array_equal(runs.cells_per_probe, cpp))
    line("rtl_gem_runs", ms, V + 9 * len(cells) + 6 * V, np_s, same)

    # ---- section 6 ----
    (kept, d), ms = timed(lambda: c.remove_high_occupancy_gems(m, call, 2), a.repeats)
    if not a.no_numpy:
        t0 = time.perf_counter()
        ci = cells.astype(np.int64)
        _, inv, per_gem = np.unique(gel[ci], return_inverse=True, return_counts=True)
        keep = per_gem[inv] <= 2
        np_s = time.perf_counter() - t0
        same = (np.array_equal(kept.cols_host(), cells[keep]) and d["high_occupancy_gems"] == int((per_gem > 2).sum())
                and d["cells_in_high_occupancy_gems"] == int((~keep).sum()))
    line("remove_high_occ", ms, 13 * len(cells) + 9 * len(cells) + 8 * kept.n_cells, np_s, same)
    occ = E.rtl_occupancy_summary(runs.cells_per_gem_hist, runs.gems_with_cells, runs.cells_per_probe)
    print("occupancy: lambda=%.6f, GEMs above 2 cells: %d with %d cells" % (occ["estimated_lambda"], d["high_occupancy_gems"],
                                                                            d["cells_in_high_occupancy_gems"]), flush=True)
    c.close()


if __name__ == "__main__":
    main()
