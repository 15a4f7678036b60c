"""Time of the aggregate detection by counts (Context.aggregates_by_counts) on the device, beside the numpy restatement on this box's CPU.
usage (GPU box): python3 scripts/bench_aggregates.py [--columns 4000000] [--cells 128000] [--probe-barcodes 1,16] [--repeats R]
                                                      [--numpy-columns 250000] [--no-ab]
The well is synthetic and seeded: 36 601 Gene Expression features followed by 140 antibodies, `columns` raw columns, of which `cells`
carry 200 Gene Expression entries and a Poisson(12) count in about 70 % of the antibodies; the others are ambient columns with a
Poisson(3) number of Gene Expression entries and a count of 1 - 2 in a Poisson(4) number of antibodies.  Six planted aggregates carry a
Poisson(900) count in 130 antibodies.  One block per number of probe barcodes (K = 25 x that):
  the median / min / max milliseconds of the timed calls (2 warm-up calls, then at least R = 10 and as many as fill half a second; host
  clock around a call that returns after the device has finished and the columns have been copied back),
  the median of the rank pass alone (crgpu_aggregates_info.rank_ms, device events around the one launch),
  the streaming bounds from the call's own bytes at 5.5 TB/s,
  the A/B of the default (one LDS slice when the table fits it, else device memory) against CRGPU_AGG_LDS_ROWS=0 (pairs and counters
  in device memory) and =4096 (as many LDS slices as it takes): three contexts in this process, created under the three settings, timed
  alternately three times each,
  and the seconds of tests/aggregates_numpy.py::aggregates_by_counts (a dense antibodies x barcodes table) and of the same computation
  in the reference's shape with pandas (pandas_by_counts below: a dense DataFrame, sort_values per antibody) on a well of
  --numpy-columns columns made the same way, with whether the device gives the same columns there.
Bytes counted.  Pass 1: 8 (V + 1) (indptr) + 4 nnz (rows) + 4 nnz_ab (antibody counts).  Column sums: 8 (V + 1) + 8 nnz + 4 V.  Sort:
8 V (keys) + 16 V P (P radix passes of 8 bits over 32 + log2 V bits).  Rank pass: 8 (V + 1) S (indptr, once per slice) + 8 nnz_ab (rows
and counts of the antibody entries; the 64-ary search's samples of the other rows are not counted), S = slices."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from cellranger_amd import engine as E  # noqa: E402

BW = 5.5e12
N_GEX, N_AB, GEX_PER_CELL = 36601, 140, 200


def timed(fn, repeats):
    """two warm-up calls, then at least `repeats` timed ones and as many as fill half a second"""
    ms, outs = [], []
    for _ in range(2):
        t0 = time.perf_counter()
        fn()
        warm = time.perf_counter() - t0
    n = max(repeats, int(0.5 / max(warm, 1e-6)) + 1)
    for _ in range(n):
        t0 = time.perf_counter()
        outs.append(fn())
        ms.append((time.perf_counter() - t0) * 1e3)
    return outs, sorted(ms)


def make_well(seed, V, n_cells):
    """CSC arrays (rows ascending inside a column) and the feature kinds"""
    rng = np.random.RandomState(seed)
    is_cell = np.zeros(V, bool)
    is_cell[rng.choice(V, n_cells, replace=False)] = True
    planted = rng.choice(np.flatnonzero(is_cell), 6, replace=False)
    n_gex = np.where(is_cell, GEX_PER_CELL, np.minimum(rng.poisson(3.0, V), 12)).astype(np.int64)
    n_ab = np.where(is_cell, rng.binomial(N_AB, 0.7, V), np.minimum(rng.poisson(4.0, V), 12)).astype(np.int64)
    n_ab[planted] = 130
    per_col = n_gex + n_ab
    indptr = np.concatenate([[0], np.cumsum(per_col)]).astype(np.int64)
    nnz = int(indptr[-1])
    col = np.repeat(np.arange(V), per_col)
    within = np.arange(nnz, dtype=np.int64) - indptr[col]
    is_ab = within >= n_gex[col]
    # ascending distinct rows: a fixed step through the section with a random offset inside the step
    k = np.where(is_ab, within - n_gex[col], within)
    n_sec = np.where(is_ab, n_ab[col], n_gex[col])
    width = np.where(is_ab, N_AB, N_GEX) // np.maximum(n_sec, 1)
    slack = np.where(is_ab, N_AB, N_GEX) - n_sec * width      # a column starts anywhere in what its steps leave free
    start = (rng.randint(0, 1 << 30, V)[col] % (slack + 1))
    feat = (np.where(is_ab, N_GEX, 0) + start + k * width + (rng.randint(0, 1 << 30, nnz) % width)).astype(np.uint32)
    data = np.ones(nnz, np.uint32)
    cell_e = is_cell[col]
    data[cell_e & ~is_ab] = rng.randint(1, 8, int((cell_e & ~is_ab).sum()))
    data[cell_e & is_ab] = rng.poisson(12.0, int((cell_e & is_ab).sum())) + 1
    amb_ab = ~cell_e & is_ab
    data[amb_ab] = rng.randint(1, 3, int(amb_ab.sum()))
    pl = np.isin(col, planted) & is_ab
    data[pl] = rng.poisson(900.0, int(pl.sum()))
    kind = np.zeros(N_GEX + N_AB, np.uint8)
    kind[N_GEX:] = 1
    return dict(indptr=indptr, indices=feat.astype(np.int32), data=data.astype(np.int32), n_features=N_GEX + N_AB, kind=kind, per_col=per_col,
                nnz_ab=int(is_ab.sum()), planted=np.sort(planted))


def pandas_by_counts(w, npb):
    """the reference's shape of the computation with pandas, written from its description: a dense barcodes x antibodies DataFrame, the
    columns below 1000 UMIs dropped, the candidates by np.argsort of the row sums, and per antibody Series.sort_values()[-K:] with a
    membership test per candidate (stable sorts here: the tie rule of the library)"""
    import pandas as pd

    import aggregates_numpy as R

    ab = np.flatnonzero(w["kind"] == R.KIND_ANTIBODY)
    df = pd.DataFrame(R.dense_rows(w["indptr"], w["indices"], w["data"], w["n_features"], ab).T, columns=["A%03d" % i for i in range(len(ab))])
    df = df.drop(labels=df.columns[np.where(df.values.sum(axis=0) < 1000)], axis=1)
    n_signal, K = len(df.columns), 25 * max(npb, 1)
    if n_signal < 5:
        return np.zeros(0, np.uint64)
    cand = df.index[np.argsort(df.values.sum(axis=1), kind="stable")[-K:]]
    found = {c: 0 for c in cand}
    for col in df.columns:
        high = df[col].sort_values(kind="stable")[-K:]
        for c in cand:
            found[c] += c in high
    return np.array(sorted(c for c in cand if found[c] >= R.min_antibodies(n_signal)), np.uint64)


def context(lds):
    old = os.environ.pop("CRGPU_AGG_LDS_ROWS", None)
    if lds is not None:
        os.environ["CRGPU_AGG_LDS_ROWS"] = lds
    try:
        c = E.Context(0)
    finally:
        os.environ.pop("CRGPU_AGG_LDS_ROWS", None)
        if old is not None:
            os.environ["CRGPU_AGG_LDS_ROWS"] = old
    return c


def load(c, w):
    V = len(w["per_col"])
    c.set_whitelist(0, np.arange(1 << int(np.ceil(np.log2(V))), dtype=np.uint32), length=16)
    seen = np.zeros(c.n_canon, np.uint32)
    seen[:V] = 1
    c.set_counts(0, 0, seen)
    m = c.assemble_matrix_dev(c.upload(np.repeat(np.arange(V, dtype=np.uint32), w["per_col"])), c.upload(w["indices"].astype(np.uint32)),
                              c.upload(w["data"].astype(np.uint32)), len(w["indices"]))
    assert m.n_barcodes == V and m.nnz == len(w["indices"])
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--columns", type=int, default=4000000)
    ap.add_argument("--cells", type=int, default=128000)
    ap.add_argument("--probe-barcodes", default="1,16")
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--numpy-columns", type=int, default=250000)
    ap.add_argument("--no-ab", action="store_true")
    a = ap.parse_args()
    V = a.columns
    w = make_well(7, V, a.cells)
    nnz = len(w["indices"])
    print("well: %d + %d features, V=%d raw columns, %d cells, nnz=%d (%d antibody entries), planted aggregates %s" % (
        N_GEX, N_AB, V, a.cells, nnz, w["nnz_ab"], w["planted"].tolist()), flush=True)
    ctxs = {"lds": context(None)}
    if not a.no_ab:
        ctxs["global"] = context("0")
        ctxs["slices"] = context("4096")
    loaded = {k: load(c, w) for k, c in ctxs.items()}
    if a.numpy_columns:      # the restatement beside the device on a smaller well made the same way (a context of its own)
        import aggregates_numpy as R

        small = make_well(7, a.numpy_columns, max(a.cells * a.numpy_columns // V, 100))
        cs = context(None)
        m_small = load(cs, small)
        for npb in (int(x) for x in a.probe_barcodes.split(",")):
            t0 = time.perf_counter()
            exp, _ = R.aggregates_by_counts(small["indptr"], small["indices"], small["data"], small["n_features"], small["kind"], npb)
            np_s = time.perf_counter() - t0
            t0 = time.perf_counter()
            exp_pd = pandas_by_counts(small, npb)
            pd_s = time.perf_counter() - t0
            outs, ms = timed(lambda: cs.aggregates_by_counts(m_small, small["kind"], npb), a.repeats)
            print("V=%d K=%d: numpy restatement (dense table) %.2f s, pandas (dense DataFrame, sort_values per antibody) %.2f s, device median %.3f ms "
                  "(x%.0f / x%.0f); same columns: %s" % (a.numpy_columns, 25 * npb, np_s, pd_s, ms[len(ms) // 2], np_s * 1e3 / ms[len(ms) // 2],
                                                       pd_s * 1e3 / ms[len(ms) // 2], np.array_equal(outs[-1][0], exp) and np.array_equal(exp_pd, exp)), flush=True)
        m_small.free()
        cs.close()
    passes = -(-(32 + int(np.ceil(np.log2(V)))) // 8)
    for npb in (int(x) for x in a.probe_barcodes.split(",")):
        def call(which):
            return ctxs[which].aggregates_by_counts(loaded[which], w["kind"], npb)

        outs, ms = timed(lambda: call("lds"), a.repeats)
        cols, info = outs[-1]
        rank = sorted(o[1]["rank_ms"] for o in outs)
        S = info["n_slices"]
        b_rank = (8 * (V + 1) * S + 8 * w["nnz_ab"]) / BW * 1e3
        b_all = (8 * (V + 1) + 4 * nnz + 4 * w["nnz_ab"] + 8 * (V + 1) + 8 * nnz + 4 * V + 8 * V + 16 * V * passes) / BW * 1e3 + b_rank
        print("K=%d: %d signal antibodies, %d slices of %d rows, %d aggregates %s (planted found: %s)" % (
            info["top_k"], info["n_signal"], S, info["rows_per_slice"], len(cols), cols.tolist(), np.isin(w["planted"], cols).all()), flush=True)
        print("    stage ms median=%.3f min=%.3f max=%.3f (%d calls) | streaming bound %.4f ms at 5.5 TB/s (x%.1f of it)" % (
            ms[len(ms) // 2], ms[0], ms[-1], len(ms), b_all, ms[len(ms) // 2] / b_all), flush=True)
        print("    rank pass alone ms median=%.3f min=%.3f max=%.3f | streaming bound %.4f ms (x%.1f of it)" % (
            rank[len(rank) // 2], rank[0], rank[-1], b_rank, rank[len(rank) // 2] / b_rank), flush=True)
        if "global" in ctxs:
            ab = {"lds": ([], []), "global": ([], []), "slices": ([], [])}
            for _ in range(3):
                for which in ("lds", "global", "slices"):
                    oo, mo = timed(lambda: call(which), a.repeats)
                    assert all(np.array_equal(o[0], cols) for o in oo)
                    rk = sorted(o[1]["rank_ms"] for o in oo)
                    ab[which][0].append(mo[len(mo) // 2])
                    ab[which][1].append(rk[len(rk) // 2])
            for what, i in (("stage", 0), ("rank pass", 1)):
                print("    A/B %s medians (ms), alternating: default %s | CRGPU_AGG_LDS_ROWS=0 %s | =4096 (as many LDS slices as it takes) %s" % (
                    what, " ".join("%.3f" % x for x in ab["lds"][i]), " ".join("%.3f" % x for x in ab["global"][i]),
                    " ".join("%.3f" % x for x in ab["slices"][i])), flush=True)
    for m in loaded.values():
        m.free()
    for c in ctxs.values():
        c.close()


if __name__ == "__main__":
    main()
