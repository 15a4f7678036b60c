"""numpy restatement of aggr's depth normalisation (the reference for cellranger_amd's crgpu_normalize_depth_dev / _plan and
crgpu_select_features_dev).

Written after mro/rna/stages/aggregator/normalize_depth/__init__.py: split() (:139-176) with _get_min_rpc_by_lt (:64-69) and
_adjust_frac_kept (:72-87); _get_new_read_pairs, _get_matrix and _update_metrics (:316-478) for ONE chunk that holds the whole
table of one GEM well; summarize_read_matrix (:229-263) with its (library type, genome) pairs numbered as classes; and
CountMatrix.select_features (lib/python/cellranger/matrix.py:886-894).  The reference stage imports martian and compiled
extensions and cannot run here, so nothing in this file is pinned against its output: the hand-computed cases of
tests/test_normalize_depth_restatement.py are the only anchor.

The one deliberate difference: np.random.seed(0); np.random.binomial(count, frac_reads_kept[library_idx]) is replaced by the
counter-based draw `kept` of tests/subsample_numpy.py, which the device reproduces bit for bit."""
import numpy as np

import subsample_numpy as S


# ---- the rates ----------------------------------------------------------------------------------------------------------------------
def plan(library_type, usable_reads, num_cells, downsample=True, targeted_aggr=False, is_targeted_lib=None, targeted_depth_factor=1.0):
    """frac_reads_kept per library"""
    usable, cells = np.array(usable_reads, dtype=np.float64), np.asarray(num_cells)
    n = len(usable)
    usable_rpc = np.divide(usable, cells.astype(np.float64), out=np.zeros(n, dtype=np.float64), where=cells > 0)
    min_rpc_by_lt = {}
    for lt, rpc in zip(library_type, usable_rpc):
        min_rpc_by_lt[lt] = min(min_rpc_by_lt.get(lt, rpc), rpc)
    if not downsample:
        return np.ones(n, dtype=float)
    frac = np.zeros(n, dtype=float)
    for i, lt in enumerate(library_type):
        if min_rpc_by_lt[lt] != 0:
            frac[i] = float(min_rpc_by_lt[lt]) / float(usable_rpc[i])
    if targeted_aggr:
        targeted = np.zeros(n, bool) if is_targeted_lib is None else np.asarray(is_targeted_lib).astype(bool)
        adjusted = [(targeted_depth_factor if targeted[i] else 1.0) * frac[i] for i in range(n)]
        if all(f <= 1.0 for f in adjusted):
            return np.array(adjusted, dtype=float)
    return frac


# ---- the stage ----------------------------------------------------------------------------------------------------------------------
def csc_of_pairs(feature, col, weight, n_cols):
    """coo_matrix((weight, (feature, col))).tocsc() with duplicates summed and zeros dropped: (indptr, indices, data)"""
    feature, col, weight = (np.asarray(x).astype(np.int64) for x in (feature, col, weight))
    order = np.lexsort((feature, col))
    feature, col, weight = feature[order], col[order], weight[order]
    head = np.ones(len(col), bool)
    head[1:] = (col[1:] != col[:-1]) | (feature[1:] != feature[:-1])
    starts = np.flatnonzero(head)
    data = np.add.reduceat(weight, starts) if len(starts) else np.zeros(0, np.int64)
    indices, cols = feature[starts], col[starts]
    nz = data != 0
    indices, cols, data = indices[nz], cols[nz], data[nz]
    indptr = np.concatenate(([0], np.cumsum(np.bincount(cols, minlength=n_cols)))).astype(np.int64)
    return indptr, indices.astype(np.int32), data.astype(np.int32)


def run(mol, frac, cell_ranks, columns, n_features, feature_class=None, n_classes=1, cell_class_mask=None, seed=0, kept_reads=None):
    """One well: mol = dict of bc (canonical ranks), lib, feature, read_count in table order; frac per library; columns = the
    barcode rank of every matrix column (ascending).  Returns the raw UMI matrix after the draw (indptr, indices, data), the read
    sums per class and per library, and `kept` per molecule."""
    bc, lib, feature, count = (np.asarray(mol[k]).astype(np.int64) for k in ("bc", "lib", "feature", "read_count"))
    frac = np.asarray(frac, np.float64)
    if np.isnan(frac).any() or (frac < 0).any() or (frac > 1).any():
        raise ValueError("p < 0, p > 1 or p is NaN")                       # numpy's binomial
    columns, cell_ranks = np.asarray(columns).astype(np.int64), np.asarray(cell_ranks).astype(np.int64)
    fclass = np.zeros(n_features, np.int64) if feature_class is None else np.asarray(feature_class).astype(np.int64)
    ccm = np.full(len(cell_ranks), (1 << n_classes) - 1, np.int64) if cell_class_mask is None else np.asarray(cell_class_mask).astype(np.int64)
    new_read_pairs = S.kept(count, lib, frac, seed) if kept_reads is None else np.asarray(kept_reads).astype(np.int64)
    keep_mol = np.flatnonzero(new_read_pairs)
    col = np.searchsorted(columns, bc)
    assert len(bc) == 0 or np.array_equal(columns[col], bc)
    indptr, indices, data = csc_of_pairs(feature[keep_mol], col[keep_mol], np.ones(len(keep_mol), np.int64), len(columns))
    # summarize_read_matrix: the read matrix restricted to the features of a class, and then to that class's cells
    mask_of_mol = np.zeros(len(bc), np.int64)                              # the classes the molecule's barcode is a cell of
    if len(cell_ranks):
        ci = np.searchsorted(cell_ranks, bc)
        ok = ci < len(cell_ranks)
        ok[ok] = cell_ranks[ci[ok]] == bc[ok]
        mask_of_mol[ok] = ccm[ci[ok]]
    raw, flt = np.zeros(n_classes, np.int64), np.zeros(n_classes, np.int64)
    for k in range(n_classes):
        mine = fclass[feature] == k
        raw[k] = new_read_pairs[mine].sum()
        flt[k] = new_read_pairs[mine & (((mask_of_mol >> k) & 1) == 1)].sum()
    n_libs = len(frac)
    return dict(indptr=indptr, indices=indices, data=data, raw_mapped_reads=raw, flt_mapped_reads=flt,
                reads_per_lib=np.bincount(lib, weights=count, minlength=n_libs).astype(np.int64),
                kept_reads_per_lib=np.bincount(lib, weights=new_read_pairs, minlength=n_libs).astype(np.int64),
                kept_molecules_per_lib=np.bincount(lib[keep_mol], minlength=n_libs).astype(np.int64),
                kept=new_read_pairs.astype(np.uint32))


# ---- CountMatrix.select_features / select_barcodes -------------------------------------------------------------------------------------
def select_features(indptr, indices, data, mask):
    """self.m[indices_to_keep, :] of a CSC for the ascending index list flatnonzero(mask): (indptr, indices, data)"""
    mask = np.asarray(mask).astype(bool)
    if len(indices) and int(np.max(indices)) >= len(mask):
        raise IndexError("row index out of range")
    new_row = np.cumsum(mask) - 1
    keep = mask[indices]
    col = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))
    out_ptr = np.concatenate(([0], np.cumsum(np.bincount(col[keep], minlength=len(indptr) - 1)))).astype(np.int64)
    return out_ptr, new_row[indices[keep]].astype(np.int32), np.asarray(data)[keep].astype(np.int32)


def select_barcodes(indptr, indices, data, cols):
    """self.m[:, cols]: (indptr, indices, data)"""
    cols = np.asarray(cols).astype(np.int64)
    lens = (indptr[cols + 1] - indptr[cols]) if len(cols) else np.zeros(0, np.int64)
    take = np.concatenate([np.arange(indptr[c], indptr[c + 1]) for c in cols]).astype(np.int64) if len(cols) else np.zeros(0, np.int64)
    return np.concatenate(([0], np.cumsum(lens))).astype(np.int64), np.asarray(indices)[take], np.asarray(data)[take]
