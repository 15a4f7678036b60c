"""Time of Context.matrix_summary on the device beside a vectorised numpy restatement on this box's CPU.
usage (GPU box): python3 scripts/bench_matrix_summary.py [--columns 600000] [--cells 10000,100000] [--classes 1,3] [--repeats R]
                                                          [--no-numpy] [--no-ab] [--once]
The well is synthetic and seeded: 36 601 features, `columns` raw columns, of which `cells` carry ~3 000 entries each (ascending
rows: a stride of 12 with a random offset inside it) and the others are ambient columns of a Poisson(4) number of entries; counts are
1 with probability 1/2 and up to 40 otherwise.  With three classes the features are dealt round robin and a cell is of one class
(every 7th of all three).  One line per (cells, classes):
  the median / min / max milliseconds of the timed calls (2 warm-up calls, then at least R = 10 and as many as fill half a second;
  host clock around a call that returns after the device has finished and the results have been copied back),
  the call's streaming bound from its own bytes at 5.5 TB/s,
  the seconds of the numpy restatement (bincount over masked entries: sum_masked / count_ge_masked of the class views, restated) with
  whether the integers are equal,
  and the A/B of the LDS-slice form against CRGPU_MS_LDS_FEATURES=0 (u64 atomics in device memory): two contexts in this process,
  created under the two settings, timed alternately three times each.
Bytes counted: 8 (V + 1) S (indptr, once per slice group) + 8 nnz (indices, data) + 4 V (cell index) + 4 V (its memset) + 4 n_cells
(masks) + 8 n_cells (list) + 16 G F (slab written and read) + 16 F (sums out) + 12 C n_cells (per-cell sums: memset, atomics read
back) + 2 * 16 * 2 C n_cells * P (keys written, then P radix passes read and write them), S = slices, G = workgroups per slice, F =
features, C = classes, P = radix passes of 8 bits over 32 + log2(2 C + 1) bits.  --once runs each configuration once and prints no
timing lines: the run a kernel trace is taken from."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cellranger_amd import engine as E  # noqa: E402

BW = 5.5e12
N_FEATURES, PER_CELL, STRIDE = 36601, 3000, 12
SLICE_MAX = (160 * 1024 - 64 - 2048) // 9


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


def make_well(seed, V, n_cells):
    rng = np.random.RandomState(seed)
    cells = np.sort(rng.choice(V, n_cells, replace=False))
    per_col = np.minimum(rng.poisson(4.0, V), STRIDE).astype(np.int64)
    per_col[cells] = PER_CELL
    indptr = np.concatenate([[0], np.cumsum(per_col)]).astype(np.int64)
    nnz = int(indptr[-1])
    within = np.arange(nnz, dtype=np.int64) - np.repeat(indptr[:-1], per_col)
    is_cell = np.zeros(V, bool)
    is_cell[cells] = True
    # ascending distinct rows: cells step by 12 with an offset inside the step, ambient columns step by 2 900 from a random start
    step = np.repeat(np.where(is_cell, STRIDE, 2900), per_col)
    start = np.repeat(np.where(is_cell, 0, rng.randint(0, 2900, V)), per_col)
    feat = (start + within * step + np.where(step == STRIDE, rng.randint(0, STRIDE, nnz), 0)).astype(np.uint32)
    assert feat.max() < N_FEATURES
    data = rng.randint(2, 41, nnz).astype(np.uint32)
    data[rng.rand(nnz) < 0.5] = 1
    return cells.astype(np.uint64), per_col, indptr, feat, data


def numpy_summary(per_col, indptr, feat, data, cells, fc, n_classes, mask):
    """the integers of the call with bincount: per feature over the class's own cells, per class, per cell"""
    V = len(per_col)
    col = np.repeat(np.arange(V), per_col)
    idx = np.full(V, -1, np.int64)
    idx[cells.astype(np.int64)] = np.arange(len(cells))
    cm = np.zeros(V, np.uint32)
    cm[cells.astype(np.int64)] = mask
    cls = fc[feat]
    own = ((cm[col] >> cls) & 1).astype(bool)
    w = data.astype(np.float64)      # exact below 2^53
    per_f = np.bincount(feat[own], weights=w[own], minlength=N_FEATURES).astype(np.uint64)
    ge2 = np.bincount(feat[own & (data >= 2)], minlength=N_FEATURES).astype(np.uint64)
    raw = np.bincount(cls, weights=w, minlength=n_classes).astype(np.uint64)
    cells_total = np.bincount(cls[own], weights=w[own], minlength=n_classes).astype(np.uint64)
    key = cls[own].astype(np.int64) * len(cells) + idx[col[own]]
    per_cell = np.bincount(key, weights=w[own], minlength=n_classes * len(cells)).astype(np.uint64).reshape(n_classes, -1)
    genes = np.bincount(key, minlength=n_classes * len(cells)).reshape(n_classes, -1)
    med = [float(np.median(per_cell[k][((mask >> k) & 1).astype(bool)])) for k in range(n_classes)]
    return per_f, ge2, raw, cells_total, per_cell, genes, med


def context(lds):
    old = os.environ.pop("CRGPU_MS_LDS_FEATURES", None)
    if lds is not None:
        os.environ["CRGPU_MS_LDS_FEATURES"] = lds
    try:
        c = E.Context(0)
    finally:
        os.environ.pop("CRGPU_MS_LDS_FEATURES", None)
        if old is not None:
            os.environ["CRGPU_MS_LDS_FEATURES"] = old
    return c


def load(c, V, per_col, feat, data, cells):
    c.set_whitelist(0, np.arange(1 << int(np.ceil(np.log2(V))), dtype=np.uint32), length=16)
    seen = np.zeros(c.n_canon, np.uint32)
    seen[:V] = 1
    c.set_counts(0, 0, seen)
    m = c.assemble_matrix_dev(c.upload(np.repeat(np.arange(V, dtype=np.uint32), per_col)), c.upload(feat), c.upload(data), len(feat))
    assert m.n_barcodes == V and m.nnz == len(feat)
    return m, c.upload(cells)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--columns", type=int, default=600000)
    ap.add_argument("--cells", default="10000,100000")
    ap.add_argument("--classes", default="1,3")
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--no-numpy", action="store_true")
    ap.add_argument("--no-ab", action="store_true")
    ap.add_argument("--once", action="store_true")
    a = ap.parse_args()
    V = a.columns
    for n_cells in (int(x) for x in a.cells.split(",")):
        cells, per_col, indptr, feat, data = make_well(7, V, n_cells)
        nnz = len(feat)
        ctxs = {"lds": context(None)}
        if not (a.no_ab or a.once):
            ctxs["global"] = context("0")
        loaded = {k: load(c, V, per_col, feat, data, cells) for k, c in ctxs.items()}
        print("well: %d features, V=%d raw columns, %d cells, nnz=%d" % (N_FEATURES, V, n_cells, nnz), flush=True)
        for n_classes in (int(x) for x in a.classes.split(",")):
            fc = (np.arange(N_FEATURES) % n_classes).astype(np.uint8)
            mask = (1 << (np.arange(n_cells) % n_classes)).astype(np.uint32)
            mask[::7] = (1 << n_classes) - 1

            def call(which):
                m, d_cells = loaded[which]
                return ctxs[which].matrix_summary(m, d_cells, feature_class=fc, n_classes=n_classes, cell_class_mask=mask)

            if a.once:
                s = call("lds")
                print("classes=%d: median counts per cell of class 0 = %.1f" % (n_classes, s.floats(0)["counts_median"]), flush=True)
                continue
            s, ms = timed(lambda: call("lds"), a.repeats)
            slices = -(-N_FEATURES // SLICE_MAX)
            G = max(1, 256 // slices)
            passes = -(-(32 + int(np.ceil(np.log2(2 * n_classes + 1)))) // 8)
            nbytes = (8 * (V + 1) * slices + 8 * nnz + 8 * V + 12 * n_cells + 16 * G * N_FEATURES + 16 * N_FEATURES + 12 * n_classes * n_cells
                      + 32 * 2 * n_classes * n_cells * passes)
            bound = nbytes / BW * 1e3
            line = "cells=%d classes=%d  ms median=%.3f min=%.3f max=%.3f (%d calls) | %.1f MB -> streaming bound %.4f ms at 5.5 TB/s (x%.1f of it)" % (
                n_cells, n_classes, ms[len(ms) // 2], ms[0], ms[-1], len(ms), nbytes / 1e6, bound, ms[len(ms) // 2] / bound)
            if not a.no_numpy:
                t0 = time.perf_counter()
                per_f, ge2, raw, cells_total, per_cell, genes, med = numpy_summary(per_col, indptr, feat, data, cells, fc, n_classes, mask)
                np_s = time.perf_counter() - t0
                sp = ctxs["lds"].matrix_summary(loaded["lds"][0], loaded["lds"][1], feature_class=fc, n_classes=n_classes, cell_class_mask=mask,
                                                per_cell=True)
                same = (np.array_equal(s.counts_per_feature, per_f) and np.array_equal(s.cells_ge2_per_feature, ge2)
                        and [c["raw_total_counts"] for c in s.classes] == raw.tolist() and [c["cells_total_counts"] for c in s.classes] == cells_total.tolist()
                        and np.array_equal(sp.counts_per_cell.to_host(), per_cell.astype(np.uint32)) and np.array_equal(sp.genes_per_cell.to_host(), genes)
                        and [s.floats(k)["counts_median"] for k in range(n_classes)] == med)
                line += " | numpy s=%.3f (x%.0f of the device; same result: %s)" % (np_s, np_s * 1e3 / ms[len(ms) // 2], same)
            print(line, flush=True)
            if "global" in ctxs:
                ab = {"lds": [], "global": []}
                for _ in range(3):
                    for which in ("lds", "global"):
                        so, mo = timed(lambda: call(which), a.repeats)
                        ab[which].append(mo[len(mo) // 2])
                        assert np.array_equal(so.counts_per_feature, s.counts_per_feature) and so.classes == s.classes
                print("    A/B medians (ms), alternating: LDS slices %s | CRGPU_MS_LDS_FEATURES=0 %s" % (
                    " ".join("%.3f" % x for x in ab["lds"]), " ".join("%.3f" % x for x in ab["global"])), flush=True)
        for m, d in loaded.values():
            m.free()
        for c in ctxs.values():
            c.close()


if __name__ == "__main__":
    main()
