"""Time of the marginal caller on the device (Context.marginal_calls) against the reference's scikit-learn loop on the same box.
usage (GPU box): python3 scripts/bench_marginal_calls.py [--repeats 7] [--cells 100000] [--guides 10000] [--gex-per-cell 300]
                 [--cmo-cells 50000] [--sklearn-rows 8] [--out profiles/marginal_calls_throughput.txt]
wells    CRISPR: --cells cells, 36 601 GEX rows + --guides guide rows.  A cell holds --gex-per-cell GEX entries (they cost the extraction
         its walk over the columns; a real well has several times as many), one or two guides at 20 - 200 UMIs, and every guide a
         background of 1 - 2 UMIs in 0.4 % of the cells.  CMO: 12 tag rows behind the GEX rows on --cmo-cells cells, every tag with a
         background in every cell and 1/12 of the cells stained.
device   one warm-up call, then --repeats calls: the host clock around Context.marginal_calls (minimum, median, maximum) and the
         library's own host clock per phase (median): extraction (count, scan, scatter, two sorts, row pointers), histogram, fit
         (seeding + Lloyd + EM are ONE kernel per (row, init): their split is not measured here), assign (predict, emit, the per-cell
         pass).  The profiler is off.
sklearn  call_presence_with_gmm_ab's own steps (GaussianMixture(n_components=2, n_init=10, covariance_type="tied", random_state=0)
         .fit + predict on log10(1 + counts)) on the dense vectors of a STATED sample of rows, one after the other as the reference's loop
         does; the time for all rows is an EXTRAPOLATION (mean of the sample x number of fitted rows) and labelled so."""
import argparse
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cellranger_amd import engine as E  # noqa: E402

N_GEX = 36601


def matrix(c, cols, rows, vals, V):
    c.set_whitelist(0, np.arange(max(4096, V), dtype=np.uint32), length=16)
    seen = np.zeros(c.n_canon, np.uint32)
    seen[:V] = 1
    c.set_counts(0, 0, seen)
    key = cols.astype(np.int64) * (1 << 20) + rows
    key, first = np.unique(key, return_index=True)      # sorted by (column, row), one entry per pair
    cols, rows, vals = (key >> 20).astype(np.uint32), (key & ((1 << 20) - 1)).astype(np.uint32), vals[first].astype(np.uint32)
    m = c.assemble_matrix_dev(c.upload(cols), c.upload(rows), c.upload(vals), len(cols))
    assert m.n_barcodes == V
    return m, cols, rows, vals


def gex_entries(rng, V, per_cell):
    cols = np.repeat(np.arange(V, dtype=np.int64), per_cell)
    rows = rng.randint(0, N_GEX, len(cols))      # a draw that repeats a (cell, gene) pair is merged: slightly fewer entries than asked for
    return cols, rows.astype(np.int64), rng.poisson(1.0, len(cols)) + 1


def crispr_well(seed, V, n_guides, per_cell):
    rng = np.random.RandomState(seed)
    gc, gr, gv = gex_entries(rng, V, per_cell)
    n_sig = rng.randint(1, 3, V)
    sc = np.repeat(np.arange(V, dtype=np.int64), n_sig)
    sr = N_GEX + rng.randint(0, n_guides, len(sc))
    sv = rng.randint(20, 200, len(sc))
    n_bg = int(0.004 * V * n_guides)
    bc, br, bv = rng.randint(0, V, n_bg).astype(np.int64), N_GEX + rng.randint(0, n_guides, n_bg), rng.randint(1, 3, n_bg)
    return np.concatenate((sc, bc, gc)), np.concatenate((sr, br, gr)), np.concatenate((sv, bv, gv)), N_GEX + n_guides      # np.unique keeps the first: the signal


def cmo_well(seed, V, k, per_cell):
    rng = np.random.RandomState(seed)
    gc, gr, gv = gex_entries(rng, V, per_cell)
    tags = rng.poisson(4.0, (V, k))
    owner = rng.randint(0, k, V)
    tags[np.arange(V), owner] += rng.poisson(500, V)
    tc, tr = np.nonzero(tags)
    return np.concatenate((tc, gc)), np.concatenate((N_GEX + tr, gr)), np.concatenate((tags[tc, tr], gv)), N_GEX + k


def stats(t):
    t = np.sort(np.array(t))
    return t[0], t[len(t) // 2], t[-1]


def device(c, m, rows, thr, nf, repeats, say):
    c.marginal_calls(m, rows, umi_threshold=thr, n_features=nf).free()
    wall, phases = [], []
    mc = None
    for _ in range(repeats):
        if mc is not None:
            mc.free()
        t = time.perf_counter()
        mc = c.marginal_calls(m, rows, umi_threshold=thr, n_features=nf)
        wall.append((time.perf_counter() - t) * 1e3)
        phases.append(mc.phase_ms)
    say("  device: %d calls, host clock per call min / median / max %.2f / %.2f / %.2f ms" % ((repeats,) + stats(wall)))
    for k in ("extract", "histogram", "fit", "assign"):
        say("    phase %-10s median %.3f ms" % (k, stats([p[k] for p in phases])[1]))
    pf = mc.per_feature
    fitted = pf["status"] == 1
    say("    rows fitted %d of %d, distinct values per fitted row median %d / max %d, cells assigned %d, rows with the histogram in LDS %d"
        % (fitted.sum(), len(rows), np.median(pf["n_distinct"][fitted]) if fitted.any() else 0, pf["n_distinct"].max(), mc.n_assigned, int(pf["in_lds"].sum())))
    return mc, stats(wall)[1]


def sklearn_loop(cols, rows, vals, V, sample, thr, say):
    from sklearn import mixture

    times, agree = [], []
    for r, want in sample:
        sel = rows == r
        counts = np.zeros(V, np.int64)
        counts[cols[sel]] = vals[sel]
        t = time.perf_counter()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            x = np.log10(1 + counts).reshape(-1, 1)
            g = mixture.GaussianMixture(n_components=2, n_init=10, covariance_type="tied", random_state=0)
            g.fit(x)
            on = (counts >= thr) & (g.predict(x) == np.argmax(g.means_))
        times.append(time.perf_counter() - t)
        agree.append(np.array_equal(np.flatnonzero(on), want))
    say("  scikit-learn %s on the same box, %d rows one after the other: %.3f s per row (min %.3f, max %.3f); calls equal to the device's on %d of %d rows"
        % (__import__("sklearn").__version__, len(sample), np.mean(times), np.min(times), np.max(times), sum(agree), len(agree)))
    return float(np.mean(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--cells", type=int, default=100000)
    ap.add_argument("--guides", type=int, default=10000)
    ap.add_argument("--gex-per-cell", type=int, default=300)
    ap.add_argument("--cmo-cells", type=int, default=50000)
    ap.add_argument("--sklearn-rows", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "marginal_calls_throughput.txt"))
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("marginal calls (Context.marginal_calls): python3 scripts/bench_marginal_calls.py " + " ".join(sys.argv[1:]))
    say("profiler off; medians of %d calls after one warm-up call" % a.repeats)
    for name, build, V, n_rows, thr in (("CRISPR", lambda: crispr_well(1, a.cells, a.guides, a.gex_per_cell), a.cells, a.guides, 3),
                                       ("CMO", lambda: cmo_well(2, a.cmo_cells, 12, a.gex_per_cell), a.cmo_cells, 12, 1)):
        cols, rows, vals, nf = build()
        c = E.Context(0)
        m, cols, rows, vals = matrix(c, cols, rows, vals, V)
        listed = np.arange(N_GEX, N_GEX + n_rows, dtype=np.uint32)
        say("%s well: %d cells, %d GEX rows + %d listed rows, %d entries in all (%d in GEX rows, %.0f per cell), %d in the listed rows, umi_threshold %d"
            % (name, V, N_GEX, n_rows, len(cols), int((rows < N_GEX).sum()), (rows < N_GEX).sum() / V, int((rows >= N_GEX).sum()), thr))
        mc, med = device(c, m, listed, thr, nf, a.repeats, say)
        cells = mc.cells_per_feature()
        fitted = np.flatnonzero(mc.per_feature["status"] == 1)
        pick = fitted[np.linspace(0, len(fitted) - 1, min(a.sklearn_rows, len(fitted))).astype(int)] if len(fitted) else []
        if len(pick):
            per_row = sklearn_loop(cols.astype(np.int64), rows, vals.astype(np.int64), V, [(N_GEX + p, cells[p].astype(np.int64)) for p in pick], thr, say)
            say("  EXTRAPOLATION to all %d fitted rows (mean of the sample x rows; not measured): %.1f s for the scikit-learn loop, against %.2f ms measured on the device"
                % (len(fitted), per_row * len(fitted), med))
        mc.free()
        m.free()
        c.close()
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
