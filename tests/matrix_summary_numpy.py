"""numpy restatement of the filtered-matrix summary metrics: report_genomes -> _report / _report_genome_agnostic_metrics
(lib/python/cellranger/rna/report_matrix.py:76-387) over views of the raw CSC matrix -- a feature mask times a barcode mask, summed
as sum_masked / count_ge_masked do (cellranger/sparse.py:36-168) -- and top_n (matrix.py:55-67).  Masks, np.add.at / bincount and
np.percentile; the moments are Python integers.  tests/test_matrix_summary_restatement.py pins it against the reference's recorded
outputs (tests/golden/matrix_summary_reference.npz, written by scripts/make_matrix_summary_golden.py) and against hand cases.

A CLASS is one (feature type, genome) pair: feature_class[f] = the class of row f (NO_CLASS: none), bit k of cell_class_mask[j] = the
j-th listed cell is a cell of class k."""
import math
from fractions import Fraction

import numpy as np

NO_CLASS = 0xFF
TOP_N = 5
MIN_COUNTS_PER_BARCODE = 2
MIN_COUNTS_PER_GENE = 1
CLASS_INT_FIELDS = ("n_features_class", "n_cells", "raw_total_counts", "union_total_counts", "union_nnz", "cells_total_counts", "cells_nnz",
                    "genes_detected", "counts_sum", "counts_sumsq_hi", "counts_sumsq_lo", "genes_sum", "genes_sumsq_hi", "genes_sumsq_lo",
                    "reads_cells")
FLOAT_FIELDS = ("counts_mean", "counts_median", "counts_cv", "counts_iqr", "counts_std", "genes_mean", "genes_median", "genes_cv", "genes_iqr",
                "genes_std", "density", "cum_frac", "dupe_frac", "reads_per_cell", "reads_cum_frac")


def robust_divide(a, b):
    """tenkit/stats.py:25-32"""
    a, b = float(a), float(b)
    return float("nan") if b == 0 else a / b


# ---- views --------------------------------------------------------------------------------------------------------------------------
def _columns(indptr):
    return np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))


def sum_masked(indptr, indices, data, n_features, row_mask, col_mask, axis):
    """sum_masked of sparse.py:36-71 without scipy: 64-bit sums"""
    col = _columns(indptr)
    keep = row_mask[indices] & col_mask[col]
    d = data[keep].astype(np.uint64)
    if axis == 0:
        out = np.zeros(len(col_mask), np.uint64)
        np.add.at(out, col[keep], d)
        return out[col_mask]
    out = np.zeros(n_features, np.uint64)
    np.add.at(out, indices[keep], d)
    return out[row_mask] if axis == 1 else int(out[row_mask].sum(dtype=np.uint64))


def count_ge_masked(indptr, indices, data, n_features, row_mask, col_mask, threshold, axis):
    """count_ge_masked of sparse.py:98-168 (the chunks only bound the reference's memory)"""
    col = _columns(indptr)
    keep = row_mask[indices] & col_mask[col] & (data >= threshold)
    if axis == 0:
        return np.bincount(col[keep], minlength=len(col_mask)).astype(np.uint64)[col_mask]
    out = np.bincount(indices[keep], minlength=n_features).astype(np.uint64)
    return out[row_mask] if axis == 1 else int(out[row_mask].sum())


def top_n(values, feature_idx, n):
    """the n largest of values[feature_idx] as [(feature, value)], by value descending, then by feature index ascending.  numpy's
    argpartition (matrix.py:64) leaves the choice among equal values at the boundary open: only the multiset of values, and the ids
    where the boundary is untied, are comparable with it"""
    order = sorted(feature_idx, key=lambda f: (-int(values[f]), int(f)))[:n]
    return [(int(f), int(values[f])) for f in order]


# ---- per-cell statistics ------------------------------------------------------------------------------------------------------------
def order_stats(x):
    """x[floor((n-1)q)] and x[min(floor((n-1)q) + 1, n-1)] of the sorted values for q = 0.25, 0.5, 0.75 (zeros for n == 0)"""
    s = np.sort(np.asarray(x))
    n, out = len(s), []
    for i in (1, 2, 3):
        if n:
            p = (n - 1) * i // 4
            out += [int(s[p]), int(s[min(p + 1, n - 1)])]
        else:
            out += [0, 0]
    return out


def lerp_percentile(n, i, a, b):
    """np.percentile(x, 25 i) from the two order statistics: numpy's linear rule"""
    t = ((n - 1) * i % 4) / 4.0
    d = float(b) - float(a)
    return float(a) + d * t if t < 0.5 else float(b) - d * (1.0 - t)


def moments(x):
    """(sum, sum of squares) as Python integers"""
    v = [int(e) for e in np.asarray(x).tolist()]
    return sum(v), sum(e * e for e in v)


def exact_std(x):
    """the population standard deviation from exact integer moments: one rounding of the quotient, one of the root"""
    n = len(x)
    s, q = moments(x)
    return math.sqrt(Fraction(n * q - s * s, n * n))


def summarize_per_barcode(a):
    """_summarize_per_barcode of report_matrix.py:316-324 in numpy's own arithmetic (std: np.std, NOT what the device reproduces)"""
    a = np.asarray(a)
    if len(a) == 0:
        nan = float("nan")
        return {"mean": nan, "median": nan, "cv": nan, "iqr": nan, "std": nan, "std_exact": nan}
    mean, std = np.mean(a), np.std(a)
    return {"mean": float(mean), "median": float(np.median(a)), "cv": robust_divide(float(std), float(mean)),
            "iqr": float(np.percentile(a, 75) - np.percentile(a, 25)), "std": float(std), "std_exact": exact_std(a)}


# ---- the summary --------------------------------------------------------------------------------------------------------------------
def summary(indptr, indices, data, n_features, cells, feature_class=None, n_classes=1, cell_class_mask=None, reads=None):
    """every integer crgpu_matrix_summary_dev reports, from masks over the raw matrix"""
    indptr, indices, data = np.asarray(indptr, np.int64), np.asarray(indices, np.int64), np.asarray(data, np.int64)
    V, cells = len(indptr) - 1, np.asarray(cells, np.int64)
    fc = np.zeros(n_features, np.uint8) if feature_class is None else np.asarray(feature_class, np.uint8)
    cm = np.full(len(cells), 0xFFFFFFFF, np.uint32) if cell_class_mask is None else np.asarray(cell_class_mask, np.uint32)
    listed = np.zeros(V, bool)
    listed[cells] = True
    everyone = np.ones(V, bool)
    counts_per_feature, cells_ge2 = np.zeros(n_features, np.uint64), np.zeros(n_features, np.uint64)
    counts_per_cell, genes_per_cell = np.zeros((n_classes, len(cells)), np.uint64), np.zeros((n_classes, len(cells)), np.uint64)
    classes = []
    for k in range(n_classes):
        rows = fc == k
        own_cells = ((cm >> np.uint32(k)) & 1).astype(bool)
        own = np.zeros(V, bool)
        own[cells[own_cells]] = True
        args = (indptr, indices, data, n_features)
        per_f = sum_masked(*args, rows, own, 1)
        counts_per_feature[rows] = per_f
        cells_ge2[rows] = count_ge_masked(*args, rows, own, MIN_COUNTS_PER_BARCODE, 1)
        x = sum_masked(*args, rows, own, 0)
        g = count_ge_masked(*args, rows, own, MIN_COUNTS_PER_GENE, 0)
        counts_per_cell[k, own_cells], genes_per_cell[k, own_cells] = x, g
        xs, xq = moments(x)
        gs, gq = moments(g)
        feats = np.flatnonzero(rows)
        n_top = min(TOP_N, len(feats))
        tc, tg = top_n(counts_per_feature, feats, n_top), top_n(cells_ge2, feats, n_top)
        classes.append(dict(
            n_features_class=int(rows.sum()), n_cells=int(own_cells.sum()), raw_total_counts=sum_masked(*args, rows, everyone, None),
            union_total_counts=sum_masked(*args, rows, listed, None), union_nnz=count_ge_masked(*args, rows, listed, 1, None),
            cells_total_counts=sum_masked(*args, rows, own, None), cells_nnz=count_ge_masked(*args, rows, own, 1, None),
            genes_detected=int(np.count_nonzero(per_f)), counts_sum=xs, counts_sumsq_hi=xq >> 64, counts_sumsq_lo=xq & (2 ** 64 - 1),
            genes_sum=gs, genes_sumsq_hi=gq >> 64, genes_sumsq_lo=gq & (2 ** 64 - 1),
            reads_cells=0 if reads is None else int(np.asarray(reads, np.uint64)[cells[own_cells]].sum(dtype=np.uint64)),
            counts_q=order_stats(x), genes_q=order_stats(g), n_top=n_top,
            top_counts_feature=[f for f, _ in tc], top_counts_value=[v for _, v in tc],
            top_cells_feature=[f for f, _ in tg], top_cells_value=[v for _, v in tg],
            counts_per_cell=x, genes_per_cell=g))
    r = None if reads is None else np.asarray(reads, np.uint64)
    return dict(n_classes=n_classes, counts_per_feature=counts_per_feature, cells_ge2_per_feature=cells_ge2, classes=classes,
                counts_per_cell=counts_per_cell, genes_per_cell=genes_per_cell, reads_all=0 if r is None else int(r.sum(dtype=np.uint64)),
                reads_union=0 if r is None else int(r[cells].sum(dtype=np.uint64)))


def class_floats(cls, reads_cells, reads_all):
    """the floats of crgpu_matrix_summary_stats from the per-cell arrays of one class, in numpy's own arithmetic; *_std is the exact
    value (np.std is compared separately), *_cv = that / mean"""
    out = {}
    for name, a in (("counts", cls["counts_per_cell"]), ("genes", cls["genes_per_cell"])):
        s = summarize_per_barcode(a)
        out[name + "_mean"], out[name + "_median"], out[name + "_iqr"] = s["mean"], s["median"], s["iqr"]
        out[name + "_std"] = s["std_exact"]
        out[name + "_cv"] = robust_divide(s["std_exact"], s["mean"])
        out[name + "_std_numpy"] = s["std"]
    out["density"] = robust_divide(cls["cells_nnz"], cls["n_features_class"] * cls["n_cells"])
    out["cum_frac"] = robust_divide(cls["cells_total_counts"], cls["raw_total_counts"])
    out["dupe_frac"] = 1 - robust_divide(cls["cells_total_counts"], reads_cells)
    out["reads_per_cell"] = robust_divide(reads_cells, cls["n_cells"])
    out["reads_cum_frac"] = robust_divide(reads_cells, reads_all)
    return out


def report(indptr, indices, data, n_features, cells, k, genome, feature_ids, feature_class=None, n_classes=1, cell_class_mask=None, reads=None,
           total_reads=None, conf_mapped_reads=None, recovered_cells=None):
    """the dict of _report (:269-387) for class k with the keys prefixed as report_genomes does (:479-499), and -- with the totals --
    the keys of _report_genome_agnostic_metrics (:76-266) that need no per-genome split of barcode_summary.h5.  Written from the
    masks alone: nothing here goes through summary()"""
    indptr, indices, data = np.asarray(indptr, np.int64), np.asarray(indices, np.int64), np.asarray(data, np.int64)
    V, cells = len(indptr) - 1, np.asarray(cells, np.int64)
    fc = np.zeros(n_features, np.uint8) if feature_class is None else np.asarray(feature_class, np.uint8)
    cm = np.full(len(cells), 0xFFFFFFFF, np.uint32) if cell_class_mask is None else np.asarray(cell_class_mask, np.uint32)
    rows = fc == k
    own = np.zeros(V, bool)
    own[cells[((cm >> np.uint32(k)) & 1).astype(bool)]] = True
    listed = np.zeros(V, bool)
    listed[cells] = True
    args = (indptr, indices, data, n_features)
    r = np.zeros(V, np.uint64) if reads is None else np.asarray(reads, np.uint64)
    d = {}
    n_cell_bcs, n_rows = int(own.sum()), int(rows.sum())
    if n_cell_bcs:
        d["filtered_gene_bc_matrix_density"] = robust_divide(count_ge_masked(*args, rows, own, 1, None), n_rows * n_cell_bcs)
        feats = np.flatnonzero(rows)
        per_gene = np.zeros(n_features, np.uint64)
        per_gene[rows] = sum_masked(*args, rows, own, 1)
        n_top = min(TOP_N, n_rows)
        d["filtered_bcs_top_genes_with_reads"] = {feature_ids[f]: v for f, v in top_n(per_gene, feats, n_top)}
        bcs_per_gene = np.zeros(n_features, np.uint64)
        bcs_per_gene[rows] = count_ge_masked(*args, rows, own, MIN_COUNTS_PER_BARCODE, 1)
        d["filtered_bcs_top_genes_with_unique_bcs"] = {feature_ids[f]: v for f, v in top_n(bcs_per_gene, feats, n_top)}
        d["filtered_bcs_total_unique_genes_detected"] = int(np.count_nonzero(per_gene))
        d["filtered_bcs_total_counts"] = int(per_gene.sum(dtype=np.uint64))
        for name, a in (("unique_genes_detected", count_ge_masked(*args, rows, own, MIN_COUNTS_PER_GENE, 0)), ("counts", sum_masked(*args, rows, own, 0))):
            s = summarize_per_barcode(a)
            for stat in ("mean", "median", "cv", "iqr"):
                d["filtered_bcs_%s_%s" % (stat, name)] = s[stat]
        filt, raw = sum_masked(*args, rows, own, None), sum_masked(*args, rows, np.ones(V, bool), None)
        d["filtered_bcs_cum_frac"] = robust_divide(filt, raw)
        n_reads, n_all = int(r[own].sum(dtype=np.uint64)), int(r.sum(dtype=np.uint64))
        have = reads is not None
        d["filtered_bcs_cdna_pcr_dupe_reads_frac"] = 1 - robust_divide(filt if have else 0, n_reads if have else 0)
        d["filtered_bcs_conf_mapped_barcoded_reads_per_filtered_bc"] = robust_divide(n_reads, n_cell_bcs)
        d["filtered_bcs_conf_mapped_barcoded_reads_cum_frac"] = robust_divide(n_reads, n_all)
        d["filtered_bcs_conf_mapped_deduped_barcoded_reads_per_filtered_bc"] = robust_divide(filt, n_cell_bcs)
        d["filtered_bcs_conf_mapped_deduped_barcoded_reads_cum_frac"] = robust_divide(filt, raw)
    out = {"%s_%s" % (genome, key): v for key, v in d.items()}
    if total_reads is not None:
        n_union = len(cells)
        in_class = fc < n_classes
        out["filtered_bcs_transcriptome_union"] = n_union
        out["multi_filtered_bcs"] = n_union
        out["reads_per_cell"] = out["multi_transcriptome_total_raw_reads_per_filtered_bc"] = robust_divide(total_reads, n_union)
        if conf_mapped_reads is not None:
            out["multi_transcriptome_total_conf_mapped_reads_per_filtered_bc"] = robust_divide(conf_mapped_reads, n_union)
        if recovered_cells is None:
            out["multi_filtered_bcs_difference_from_recovered_cells"] = 0
            out["multi_filtered_bcs_relative_difference_from_recovered_cells"] = 0
        else:
            out["multi_filtered_bcs_difference_from_recovered_cells"] = int(n_union) - int(recovered_cells)
            out["multi_filtered_bcs_relative_difference_from_recovered_cells"] = robust_divide(n_union - recovered_cells, recovered_cells)
        out["multi_filtered_gene_bc_matrix_density"] = robust_divide(count_ge_masked(*args, in_class, listed, 1, None), int(in_class.sum()) * n_union)
        out["%s_total_raw_reads_per_filtered_bc" % genome] = robust_divide(total_reads, n_union)
        if conf_mapped_reads is not None:
            out["%s_total_conf_mapped_reads_per_filtered_bc" % genome] = robust_divide(conf_mapped_reads, n_union)
        out["%s_total_conf_mapped_deduped_barcoded_reads_per_filtered_bc" % genome] = robust_divide(sum_masked(*args, in_class, listed, None), n_union)
        usable = int(r[listed].sum(dtype=np.uint64))
        frac = robust_divide(usable, int(r.sum(dtype=np.uint64)))
        out["multi_filtered_bcs_conf_mapped_barcoded_reads_cum_frac"] = out["feature_reads_in_cells"] = frac
        out["multi_transcriptome_usable_reads_frac"] = out["frac_feature_reads_usable"] = robust_divide(usable, total_reads)
        out["multi_usable_reads"] = usable
        out["multi_usable_reads_per_filtered_bc"] = out["feature_reads_usable_per_cell"] = robust_divide(usable, n_union)
    return out


# ---- fixtures -----------------------------------------------------------------------------------------------------------------------
def hand_matrix():
    """6 features x 8 columns, two classes: features 0 1 2 -> class 0, 3 4 -> class 1, 5 -> no class.  Cells: columns 1 (class 0), 3 (both),
    6 (class 1); class-0 entries of exactly 1 (row 1, column 1) and exactly 2 (row 0, column 3)."""
    cols = [{0: 3, 5: 9}, {0: 5, 1: 1, 3: 7}, {}, {0: 2, 2: 4, 3: 1, 4: 6, 5: 2}, {1: 8, 4: 1}, {2: 1}, {0: 11, 3: 2, 4: 2}, {5: 4}]
    indptr = np.cumsum([0] + [len(c) for c in cols]).astype(np.int64)
    indices = np.array([f for c in cols for f in sorted(c)], np.int32)
    data = np.array([c[f] for c in cols for f in sorted(c)], np.int32)
    return dict(indptr=indptr, indices=indices, data=data, n_features=6, n_classes=2, feature_class=np.array([0, 0, 0, 1, 1, NO_CLASS], np.uint8),
                cells=np.array([1, 3, 6], np.uint64), cell_class_mask=np.array([1, 3, 2], np.uint32),
                reads=np.array([20, 30, 0, 40, 15, 2, 50, 7], np.uint32))


def make_matrix(seed, n_features=300, n_cols=1000, entries=20, n_cells=200, n_classes=3, no_class=0.1, max_count=40, empty=0.05, overlap=True):
    """a seeded raw matrix: ~entries rows per column (cells carry five times as many), classes dealt to the features at random with
    a share in no class, cell masks that overlap, reads >= the column's UMIs"""
    rng = np.random.RandomState(seed)
    fc = rng.randint(0, n_classes, n_features).astype(np.uint8)
    fc[rng.rand(n_features) < no_class] = NO_CLASS
    cells = np.sort(rng.choice(n_cols, n_cells, replace=False)).astype(np.uint64)
    is_cell = np.zeros(n_cols, bool)
    is_cell[cells.astype(np.int64)] = True
    per_col = np.minimum(rng.poisson(np.where(is_cell, 5 * entries, entries)), n_features)
    per_col[rng.rand(n_cols) < empty] = 0
    indptr = np.concatenate(([0], np.cumsum(per_col))).astype(np.int64)
    indices = np.concatenate([np.sort(rng.choice(n_features, k, replace=False)) for k in per_col] + [np.zeros(0, np.int64)]).astype(np.int32)
    data = rng.randint(1, max_count + 1, len(indices)).astype(np.int32)
    data[rng.rand(len(data)) < 0.5] = 1
    if overlap:
        mask = rng.randint(1, 1 << n_classes, n_cells).astype(np.uint32)
        mask[rng.rand(n_cells) < 0.05] = 0      # a listed cell of no class
    else:
        mask = (1 << rng.randint(0, n_classes, n_cells)).astype(np.uint32)
    sums = np.zeros(n_cols, np.uint64)
    np.add.at(sums, _columns(indptr), data.astype(np.uint64))
    reads = (sums + rng.randint(0, 50, n_cols).astype(np.uint64)).astype(np.uint32)
    return dict(indptr=indptr, indices=indices, data=data, n_features=n_features, n_classes=n_classes, feature_class=fc, cells=cells,
                cell_class_mask=mask, reads=reads)


def wave_matrix(big=False):
    """empty columns, a column of 65 and one of 300 entries (the wave loop), feature 7 present in every cell; big: data up to 2^31 - 1, so
    that the sum of feature 7 passes 2^32 (no per-cell sum does: every cell keeps one large entry).  The cells 1, 10 and 11 lie in
    one group of 16 columns and are cells of feature 7's class: the three entries one workgroup adds to its counter reach
    3 (2^31 - 1) >= 2^32 on their own"""
    rng = np.random.RandomState(5)
    n_features, n_cols = 400, 64
    per_col = rng.randint(0, 30, n_cols)
    per_col[[3, 4, 20, 41]] = 0
    per_col[10], per_col[33] = 65, 300
    cells = np.array([1, 10, 11, 33, 40, 50, 63], np.uint64)
    rows = []
    for c in range(n_cols):
        r = set(rng.choice(n_features, per_col[c], replace=False).tolist()) if per_col[c] else set()
        if c in cells.tolist() and 7 not in r:
            r = set(list(r)[: max(len(r) - 1, 0)]) | {7}
        rows.append(sorted(r))
    indptr = np.cumsum([0] + [len(r) for r in rows]).astype(np.int64)
    indices = np.array([f for r in rows for f in r], np.int32)
    data = rng.randint(1, 9, len(indices)).astype(np.int32)
    if big:
        col = _columns(indptr)
        data[(indices == 7) & np.isin(col, cells.astype(np.int64))] = 2 ** 31 - 1
    fc = (np.arange(n_features) % 2).astype(np.uint8)
    fc[5] = NO_CLASS
    return dict(indptr=indptr, indices=indices, data=data, n_features=n_features, n_classes=2, feature_class=fc, cells=cells,
                cell_class_mask=np.array([3, 3, 3, 3, 2, 3, 3], np.uint32), reads=None)


def golden_fixtures():
    """the fixtures the reference's outputs are recorded for (row sums of the reference are int32: data stays small here)"""
    return {"hand": hand_matrix(), "mid": make_matrix(11), "wave": wave_matrix(False)}


def run(fx, **kw):
    args = dict(feature_class=fx["feature_class"], n_classes=fx["n_classes"], cell_class_mask=fx["cell_class_mask"], reads=fx["reads"])
    args.update(kw)
    return summary(fx["indptr"], fx["indices"], fx["data"], fx["n_features"], fx["cells"], **args)
