#!/usr/bin/env python
"""Record tests/golden/pca_reference.npz: what the reference's own irlb and stats functions give on the wells of tests/pca_numpy.py.

    python scripts/make_pca_golden.py --reference DIR

DIR is a checkout of the reference.  Its lib/python/cellranger/analysis/irlb.py and stats.py are loaded BY PATH (numpy, scipy and
scikit-learn 1.7.2's sparsefuncs are all they need); pca.py pulls in modules that cannot be imported without the rest of the product,
so the body of run_pca (pca.py:49-209), normalize_and_transpose (212-229), select_axes_above_threshold (matrix.py:788-810) and the retry
of the stage (mro/rna/stages/analyzer/run_pca/__init__.py:57-80) are restated here around them on a scipy CSC matrix.

Per fixture <f>:
  <f>_transformed, _components, _variance_explained, _dispersion, _features_selected (feature indices in the order of org_cols_used),
  <f>_d, _it, _mprod, _retried, _n_components, _n_thresholded_bcs      the PCA tuple and what the tests compare exactly
  <f>_mu, _var, _disp_thr                                             the inputs and the output of get_normalized_dispersion
  <f>_B0, <f>_B1                                                      the B of the first SVD and of the first restarted one (if any)
  <f>_mov_d, _mov_variance_explained, _mov_components, _mov_transformed, _mov_dispersion
        the movement of the reference itself: the largest difference between the same computation under three orders of the cells
        (identity and two seeded permutations; signs aligned, rows put back), relative to the largest finite entry of the quantity,
        and never below 2^-53, one rounding of that entry.  The tests allow 16 times this.

A fixture is REJECTED when two neighbouring dispersions in the feature order differ by less than 1e-9 relative without being bit-equal
in all three orders, or when some |R_i| lies within 1e-6 relative of tol * smax at a restart (either would let a last bit decide a
discrete output).  The number rejected is printed; more than a quarter is an error: choose other seeds in tests/pca_numpy.py."""
import argparse
import importlib.util
import os
import sys

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import pca_numpy as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "pca_reference.npz")
ORDER_SEEDS = (None, 101, 202)
ROUNDING = 2.0 ** -53


def load_by_path(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class Matrix:
    """the three members of CountMatrix that stats.normalize_by_umi reads"""

    def __init__(self, m):
        self.m = sp.csc_matrix(m)

    def get_counts_per_bc(self):
        return np.squeeze(np.asarray(self.m.sum(axis=0)))

    def get_counts_per_feature(self):
        return np.squeeze(np.asarray(self.m.sum(axis=1)))

    def select(self, feats=None, bcs=None):
        m = self.m
        if bcs is not None:
            m = m[:, bcs]
        if feats is not None:
            m = m[feats, :]
        return Matrix(m)


def normalize_and_transpose(stats, matrix):
    m = stats.normalize_by_umi(matrix)
    m.data = np.log2(1 + m.data)
    m = m.T
    c, v = stats.summarize_columns(m)
    v[np.where(v == 0.0)] = 1.0
    return m, c, np.sqrt(v)


def run_pca(stats, irlb_mod, matrix, pca_features, pca_bc_indices, n_pca_components, min_count_threshold, record):
    from sklearn.utils import sparsefuncs

    nonzero_bcs = np.flatnonzero(matrix.get_counts_per_bc() > min_count_threshold)
    thr = matrix.select(bcs=nonzero_bcs)
    thresholded_features = np.flatnonzero(np.atleast_1d(thr.get_counts_per_feature()) > min_count_threshold)
    thr = thr.select(feats=thresholded_features)
    if len(nonzero_bcs) == 0 or len(thresholded_features) == 0:
        raise R.NullAxisMatrix()
    bcs_dim, features_dim = thr.m.shape[1], thr.m.shape[0]
    if pca_bc_indices is None:
        pca_bc_indices = np.arange(bcs_dim)
    pca_bcs = len(pca_bc_indices)
    if pca_features is None or pca_features > features_dim:
        pca_features = features_dim
    m = stats.normalize_by_umi(thr)
    mu, var = stats.summarize_columns(m.T)
    with np.errstate(divide="ignore", invalid="ignore"):
        dispersion = stats.get_normalized_dispersion(mu.squeeze(), var.squeeze())
    pca_feature_indices = np.argsort(dispersion, kind="stable")[-pca_features:]
    likely_matrix_rank = min(pca_features, pca_bcs)
    if likely_matrix_rank < n_pca_components:
        if min_count_threshold == R.DEFAULT_RUNPCA_THRESHOLD:
            raise R.MatrixRankTooSmall("Matrix rank is too small")
        n_pca_components = likely_matrix_rank
    pca_mat = thr.select(bcs=pca_bc_indices).select(feats=pca_feature_indices)
    pca_norm_mat, pca_center, pca_scale = normalize_and_transpose(stats, pca_mat)
    sparsefuncs.inplace_column_scale(pca_norm_mat, 1.0 / np.atleast_1d(pca_scale.squeeze()))
    pca_center /= pca_scale
    with Hooks(record):
        _, d, v, it, mprod = irlb_mod.irlb(pca_norm_mat, n_pca_components, center=np.atleast_1d(pca_center.squeeze()), random_state=0)
    full_norm_mat, full_center, full_scale = normalize_and_transpose(stats, matrix)
    sparsefuncs.inplace_column_scale(full_norm_mat, 1.0 / np.atleast_1d(full_scale.squeeze()))
    org_cols_used = [thresholded_features[x] for x in pca_feature_indices]
    transformed = full_norm_mat[:, org_cols_used].dot(v) - (full_center / full_scale)[:, org_cols_used].dot(v)
    components = np.zeros((n_pca_components, matrix.m.shape[0]))
    components[:, org_cols_used] = v.T
    variance_explained = np.square(d) / ((len(pca_bc_indices) - 1) * len(pca_feature_indices))
    full_dispersion = np.full(matrix.m.shape[0], np.nan)
    full_dispersion[thresholded_features] = dispersion
    return dict(transformed=np.asarray(transformed), components=components, variance_explained=variance_explained, dispersion=full_dispersion,
                features_selected=np.array(org_cols_used, dtype=np.int64), d=d, it=it, mprod=mprod, n_components=n_pca_components,
                mu=mu.squeeze(), var=var.squeeze(), disp_thr=dispersion, n_thresholded_bcs=bcs_dim, thresholded_bcs=nonzero_bcs)


class Hooks:
    """while irlb runs: every B handed to np.linalg.svd, with R = fn * U[m_b - 1] (fn is the last norm taken before the SVD) and smax"""

    def __init__(self, record):
        self.record, self.last_norm, self.smax = record, None, None

    def __enter__(self):
        self.svd, self.norm = np.linalg.svd, np.linalg.norm

        def norm(x, *a, **k):
            self.last_norm = self.norm(x, *a, **k)
            return self.last_norm

        def svd(b, *a, **k):
            s = self.svd(b, *a, **k)
            self.smax = s[1][0] if self.smax is None else max(s[1][0], self.smax)
            self.record.append(dict(B=np.array(b), R=self.last_norm * s[0][b.shape[0] - 1, :], smax=self.smax))
            return s

        np.linalg.svd, np.linalg.norm = svd, norm
        return self

    def __exit__(self, *exc):
        np.linalg.svd, np.linalg.norm = self.svd, self.norm


def run_stage(stats, irlb_mod, dense, kw, record):
    matrix = Matrix(dense)
    try:
        return run_pca(stats, irlb_mod, matrix, kw.get("pca_features"), kw.get("pca_bc_indices"), kw["n_components"], 2, record), False
    except (R.NullAxisMatrix, R.MatrixRankTooSmall):
        del record[:]
        return run_pca(stats, irlb_mod, matrix, kw.get("pca_features"), kw.get("pca_bc_indices"), kw["n_components"], 0, record), True


def rel_movement(runs, key, scale_of=None):
    ref = runs[0][key]
    fin = np.isfinite(ref)
    for r in runs[1:]:      # the same NaN and infinity places in every order, or the orders are not comparable
        assert np.array_equal(np.isnan(r[key]), np.isnan(ref)) and np.array_equal(r[key][~fin & ~np.isnan(ref)], ref[~fin & ~np.isnan(ref)]), key
    scale = np.abs(ref[fin]).max() if fin.any() else 1.0
    mov = max([np.abs(r[key][fin] - ref[fin]).max() if fin.any() else 0.0 for r in runs[1:]] + [0.0])
    return max(mov / scale, ROUNDING) if scale > 0 else ROUNDING


def one_fixture(name, stats, irlb_mod, out):
    """-> the reason of a rejection, or None"""
    dense = R.FIXTURES[name]["make"]()
    n_bcs = dense.shape[1]
    runs, records, retried = [], [], []
    base_cells = None
    for seed in ORDER_SEEDS:
        order = np.arange(n_bcs) if seed is None else np.random.RandomState(seed).permutation(n_bcs)
        mat = dense[:, order]
        probe, _ = run_stage(stats, irlb_mod, mat, dict(n_components=R.FIXTURES[name]["n_components"], pca_features=R.FIXTURES[name].get("pca_features")), [])
        kw = R.fixture_args(name, probe["n_thresholded_bcs"])
        if "pca_bc_indices" in kw:      # the same cells under every order
            if base_cells is None:
                base_cells = set(order[probe["thresholded_bcs"][kw["pca_bc_indices"]]].tolist())
            kw["pca_bc_indices"] = np.flatnonzero([order[c] in base_cells for c in probe["thresholded_bcs"]])
        rec = []
        r, again = run_stage(stats, irlb_mod, mat, kw, rec)
        back = np.empty(n_bcs, dtype=np.int64)
        back[order] = np.arange(n_bcs)
        r["transformed"] = r["transformed"][back]
        if runs:
            signs, cos = R.align_signs(r["components"], runs[0]["components"])
            assert cos.min() > 0.99, "%s: a component turns under a permutation of the cells (cosine %.6f)" % (name, cos.min())
            r["components"] = r["components"] * signs[:, None]
            r["transformed"] = r["transformed"] * signs[None, :]
        runs.append(r)
        records.append(rec)
        retried.append(again)
    first = runs[0]
    # rejection 1: neighbours in the feature order
    with np.errstate(invalid="ignore", divide="ignore"):
        for r in runs:
            d = r["disp_thr"]
            srt = d[np.argsort(d, kind="stable")]
            a, b = srt[:-1], srt[1:]
            close = np.isfinite(a) & np.isfinite(b) & (np.abs(b - a) < 1e-9 * np.maximum(np.abs(a), np.abs(b))) & (a != b)
            if close.any():
                return "two neighbouring dispersions differ by less than 1e-9 relative"
        for r in runs[1:]:
            d0, d1 = first["disp_thr"], r["disp_thr"]
            order0 = np.argsort(d0, kind="stable")
            ties = np.flatnonzero((d0[order0][1:] == d0[order0][:-1]) | (np.isnan(d0[order0][1:]) & np.isnan(d0[order0][:-1])))
            for t in ties:
                x, y = d1[order0[t]], d1[order0[t + 1]]
                if not (x == y or (np.isnan(x) and np.isnan(y))):
                    return "a tie of the dispersions is not a tie in every order"
    # rejection 2: the convergence count
    for rec in records:
        for step in rec:
            nu = first["n_components"]
            lim = R.TOL * step["smax"]
            if (np.abs(np.abs(step["R"][:nu]) - lim) < 1e-6 * lim).any():
                return "an |R_i| lies within 1e-6 relative of tol * smax"
    for r, again in zip(runs[1:], retried[1:]):      # with neither rejection, no discrete output may move with the order of the cells
        assert again == retried[0] and r["it"] == first["it"] and r["mprod"] == first["mprod"] and np.array_equal(r["features_selected"], first["features_selected"]), \
            "%s: a discrete output moves with the order of the cells" % name
    for key in ("transformed", "components", "variance_explained", "dispersion", "features_selected", "d", "mu", "var", "disp_thr"):
        out["%s_%s" % (name, key)] = first[key]
    for key in ("it", "mprod", "n_components", "n_thresholded_bcs"):
        out["%s_%s" % (name, key)] = np.int64(first[key])
    out[name + "_retried"] = np.int64(retried[0])
    for i, step in enumerate(records[0][:2]):
        out["%s_B%d" % (name, i)] = step["B"]
    for key in ("d", "variance_explained", "components", "transformed", "dispersion"):
        out["%s_mov_%s" % (name, key)] = np.float64(rel_movement(runs, key))
    print("%-12s %s retried %d components %d it %d mprod %d; movement d %.2g ve %.2g components %.2g transformed %.2g dispersion %.2g"
          % (name, dense.shape, retried[0], first["n_components"], first["it"], first["mprod"], out[name + "_mov_d"], out[name + "_mov_variance_explained"],
             out[name + "_mov_components"], out[name + "_mov_transformed"], out[name + "_mov_dispersion"]))
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="a checkout of the reference (two of its files are loaded by path)")
    a = ap.parse_args()
    import sklearn

    assert sklearn.__version__ == "1.7.2", "the reference is scikit-learn 1.7.2, this is %s" % sklearn.__version__
    ana = os.path.join(a.reference, "lib", "python", "cellranger", "analysis")
    stats = load_by_path("crgpu_ref_stats", os.path.join(ana, "stats.py"))
    irlb_mod = load_by_path("crgpu_ref_irlb", os.path.join(ana, "irlb.py"))
    out, rejected = {}, []
    for name in R.FIXTURES:
        part = {}
        why = one_fixture(name, stats, irlb_mod, part)
        if why:
            print("%-12s REJECTED: %s" % (name, why))
            rejected.append((name, why))
        else:
            out.update(part)
    # the chain: the reference's projection of the three-group well, for engine.run_kmeans
    dense, group = R.chain_well()
    r, _ = run_stage(stats, irlb_mod, dense, dict(n_components=R.CHAIN["n_components"]), [])
    out["chain_transformed"], out["chain_group"] = r["transformed"], group.astype(np.int32)
    print("fixtures: %d, rejected: %d %s" % (len(R.FIXTURES), len(rejected), rejected))
    if 4 * len(rejected) > len(R.FIXTURES):
        raise SystemExit("more than a quarter of the fixtures rejected: choose other seeds in tests/pca_numpy.py")
    np.savez_compressed(OUT, **out)
    print("%s: %d bytes" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
