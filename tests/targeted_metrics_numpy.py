"""Restatements of CALCULATE_TARGETED_METRICS (mro/rna/stages/targeted/calculate_targeted_metrics/__init__.py) in numpy / pandas,
for the tests of the targeted-metrics entry points.  No GPU, no library.

  tallies         collapse_feature_counts' chunk function (lib/python/cellranger/pandas_utils.py:600-637) over molecule arrays: the
                  same np.isin / np.add.at calls.  pandas_utils itself needs h5py and cannot be imported in the test image, so the
                  tallies are pinned by hand-computed cases (hand_molecules), as tests/subsample_numpy.py does.
  rpu_stats       get_feature_summary_df's columns and get_mean_per_gene_rpu_metrics (:220-301): literally the reference's pandas
                  calls, plus the gene counts of get_enrichment_metrics (:167-215).
  em_tied / fit   scikit-learn's GaussianMixture(covariance_type="tied") for 1-D data as fit_2comp_gmm (targeted/gmm.py:26-112)
                  drives it: initialisation from the given weights / means / precision, e-step, m-step with reg_covar 1e-6 and
                  nk + 10 eps, the lower bound = mean logsumexp under the PREVIOUS parameters, stop at |change| < 1e-3 or after
                  100 iterations; 1 + 5151 starts, the first of equal likelihoods wins.
  fit_enrichments the guards of gmm.py:145-169 around it, ClassStats from values >= threshold.
  targeted_metrics  the summary dict of join() from tallies, flags and the caller's numbers.
"""
import math
import warnings

import numpy as np
import pandas as pd
import scipy.stats
from scipy.special import logsumexp

MIN_UMIS = 10
MIN_RPU_THRESHOLD = 2.5
MIN_OFFTARGET_GENES = 30
RPU_NUM_TRIES = 100
N_STARTS = 1 + (RPU_NUM_TRIES + 1) * (RPU_NUM_TRIES + 2) // 2      # 5152
FIT_KEYS = ("log_rpu_threshold", "mu_high", "mu_low", "sd_high", "sd_low", "alpha_high", "alpha_low")
CLASS_KEYS = ("n_targeted_enriched", "n_targeted_not_enriched", "n_offtgt_enriched", "n_offtgt_not_enriched")


def robust_divide(a, b):
    return float("nan") if b == 0 else float(a) / float(b)


# ---- 1. the tallies ---------------------------------------------------------------------------------------------------------------
def tallies(mol, n_features, libs, cell_ranks):
    """mol: dict of bc, lib, feature, read_count (Counts.molecules()); libs: filter_library_idx; cell_ranks: the union of the
    pass-filter barcodes of those libraries -> num_umis, num_reads, num_umis_cells, num_reads_cells (u64 per feature)"""
    read_counts_by_index = np.zeros(n_features, dtype=np.uint64)
    umi_counts_by_index = np.zeros(n_features, dtype=np.uint64)
    read_counts_in_cells_by_index = np.zeros(n_features, dtype=np.uint64)
    umi_counts_in_cells_by_index = np.zeros(n_features, dtype=np.uint64)
    idx_mol = np.ones(len(mol["bc"]), dtype="bool")
    idx_mol &= np.isin(mol["lib"], list(libs))
    is_cell = np.isin(mol["bc"], cell_ranks)
    is_cell = is_cell[idx_mol]
    feature_indices = mol["feature"][idx_mol]
    read_counts = mol["read_count"][idx_mol].astype(np.uint64)
    np.add.at(umi_counts_by_index, feature_indices, np.ones(feature_indices.shape[0], dtype=np.uint64))
    np.add.at(read_counts_by_index, feature_indices, read_counts)
    feature_indices = feature_indices[is_cell]
    read_counts = read_counts[is_cell]
    np.add.at(umi_counts_in_cells_by_index, feature_indices, np.ones(feature_indices.shape[0], dtype=np.uint64))
    np.add.at(read_counts_in_cells_by_index, feature_indices, read_counts)
    return umi_counts_by_index, read_counts_by_index, umi_counts_in_cells_by_index, read_counts_in_cells_by_index


def hand_molecules():
    """eight molecules, two libraries, four features, barcodes 2 and 5 are cells; the expected tallies are worked out by hand"""
    mol = dict(bc=np.array([1, 2, 2, 2, 5, 5, 7, 7], np.uint32), lib=np.array([0, 0, 0, 1, 0, 1, 0, 1], np.uint8),
               feature=np.array([0, 0, 0, 3, 3, 0, 1, 1], np.uint32), read_count=np.array([4, 1, 2, 7, 5, 9, 3, 6], np.uint32))
    cells = np.array([2, 5], np.uint32)
    expect = {
        (0,): ([3, 1, 0, 1], [7, 3, 0, 5], [2, 0, 0, 1], [3, 0, 0, 5]),
        (1,): ([1, 1, 0, 1], [9, 6, 0, 7], [1, 0, 0, 1], [9, 0, 0, 7]),
        (0, 1): ([4, 2, 0, 2], [16, 9, 0, 12], [3, 0, 0, 2], [12, 0, 0, 12]),
    }
    return mol, cells, 4, expect


# ---- 2. reads-per-UMI statistics and gene counts ----------------------------------------------------------------------------------
def feature_summary_df(num_umis, num_reads, num_umis_cells, num_reads_cells, is_targeted, is_gex=None):
    """get_feature_summary_df (:270-301) behind collapse_feature_counts: GEX rows only, the four ratio columns"""
    df = pd.DataFrame({"num_umis": np.asarray(num_umis, np.uint64), "num_reads": np.asarray(num_reads, np.uint64),
                       "num_umis_cells": np.asarray(num_umis_cells, np.uint64), "num_reads_cells": np.asarray(num_reads_cells, np.uint64),
                       "feature_idx": np.arange(len(num_umis))})
    df["is_targeted"] = np.asarray(is_targeted).astype(bool)
    if is_gex is not None:
        df = df[np.asarray(is_gex).astype(bool)].copy()
    with np.errstate(divide="ignore", invalid="ignore"):
        df["mean_reads_per_umi"] = df["num_reads"].divide(other=df["num_umis"])
        df["mean_reads_per_umi_log10"] = np.log10(df["mean_reads_per_umi"])
        df["mean_reads_per_umi_cells"] = df["num_reads_cells"].divide(other=df["num_umis_cells"])
        df["mean_reads_per_umi_cells_log10"] = np.log10(df["mean_reads_per_umi_cells"])
    return df


def mean_per_gene_rpu_metrics(pfm):
    """get_mean_per_gene_rpu_metrics (:220-267), is_spatial False"""
    per_gene_rpu_metrics = {}
    for targeting in [True, False]:
        target_suffix = "on_target" if targeting else "off_target"
        for in_cells in [True, False]:
            in_cells_suffix = "_cells" if in_cells else ""
            reads_per_umi = pfm[(pfm["is_targeted"] == targeting) & (pfm["num_umis_cells"] >= MIN_UMIS)][f"mean_reads_per_umi{in_cells_suffix}"]
            if reads_per_umi.shape[0] == 0:
                mean_rpu = cv_rpu = median_rpu = iqrnorm_rpu = perc80_rpu = 0.0
            else:
                with warnings.catch_warnings():      # (a selection of NaNs only: numpy warns about the empty slice)
                    warnings.simplefilter("ignore")
                    mean_rpu = reads_per_umi.mean(skipna=True)
                    std_rpu = reads_per_umi.std(skipna=True)
                    cv_rpu = robust_divide(std_rpu, mean_rpu)
                    median_rpu = reads_per_umi.median(skipna=True)
                    iqrnorm_rpu = robust_divide(reads_per_umi.quantile(0.75) - reads_per_umi.quantile(0.25), median_rpu)
                    perc80_rpu = reads_per_umi.quantile(0.80)
            for name, v in (("mean", mean_rpu), ("cv", cv_rpu), ("median", median_rpu), ("iqrnorm", iqrnorm_rpu), ("perc80", perc80_rpu)):
                per_gene_rpu_metrics[f"{name}_reads_per_umi_per_gene{in_cells_suffix}_{target_suffix}"] = float(v)
    return per_gene_rpu_metrics


def float_bounds(pfm):
    """key -> (rel, abs), both in units of 2^-52: crgpu_targeted_rpu_stats must meet pandas' mean / cv within
    rel * 2^-52 * |reference| + abs * 2^-52; every other statistic is compared bit for bit.  Derived from the two summation schemes,
    not from what is observed (u = 2^-53):
      mean  both sides add the same n non-negative quotients, the library in numpy's pairwise order over the n values, pandas in
            that order over the frame with the skipped NaNs replaced by zeros (another grouping).  Any order of adding n
            non-negative terms is within (n - 1) u of the exact sum, the two sums within 2 (n - 1) u of each other, the division
            rounds once on either side: rel = n.
      std   sqrt(sum((avg - x)^2) / (n - 1)).  The two avg differ by d <= n 2^-52 avg; the vector (avg - x) moves by d in every
            component, its norm by at most d sqrt(n), the std by d sqrt(n / (n - 1)) <= 1.5 d.  With the same avg: each square
            carries three roundings, the two orders of adding n non-negative squares differ by 2 (n - 1) u, the division rounds once
            on either side; the square root halves that and rounds once: (n + 4) / 2 + 1, relative.
      cv    std / mean: rel = (n + 4) / 2 + 1 + n + 1 (std, mean, the division), abs = 1.5 d / avg <= 2 n."""
    out = {}
    for targeting in [True, False]:
        for in_cells in [True, False]:
            suffix = ("_cells" if in_cells else "") + ("_on_target" if targeting else "_off_target")
            x = pfm[(pfm["is_targeted"] == targeting) & (pfm["num_umis_cells"] >= MIN_UMIS)]["mean_reads_per_umi" + ("_cells" if in_cells else "")]
            x = x.to_numpy()
            n = int((~np.isnan(x)).sum())
            out["mean_reads_per_umi_per_gene" + suffix] = (float(n), 0.0)
            out["cv_reads_per_umi_per_gene" + suffix] = ((n + 4) / 2.0 + 1 + n + 1, 2.0 * n)
    return out


def gene_counts(pfm):
    """the counts of get_enrichment_metrics (:167-215), is_spatial False"""
    t, u = pfm["is_targeted"], pfm["num_umis_cells"]
    nd_on, nd_off = int(((t == 1) & (u == 0)).sum()), int(((t == 0) & (u == 0)).sum())
    nq_on, nq_off = int(((t == 1) & (u < MIN_UMIS)).sum()), int(((t == 0) & (u < MIN_UMIS)).sum())
    n_on, n_off = int(pfm[t == True].shape[0]), int(pfm[t == False].shape[0])      # noqa: E712
    return {"num_genes_not_detected_on_target": nd_on, "num_genes_not_detected_off_target": nd_off,
            "num_genes_detected_on_target": n_on - nd_on, "num_genes_detected_off_target": n_off - nd_off,
            "num_genes_not_quantifiable_on_target": nq_on, "num_genes_not_quantifiable_off_target": nq_off,
            "num_genes_on_target": n_on, "num_genes_off_target": n_off,
            "num_genes_quantifiable_on_target": n_on - nq_on, "num_genes_quantifiable_off_target": n_off - nq_off}


def rpu_stats(num_umis, num_reads, num_umis_cells, num_reads_cells, is_targeted, is_gex=None):
    """what crgpu_targeted_rpu_stats returns: the 20 statistics, the saturation, the gene counts and the quantifiable list"""
    pfm = feature_summary_df(num_umis, num_reads, num_umis_cells, num_reads_cells, is_targeted, is_gex)
    out = mean_per_gene_rpu_metrics(pfm)
    total_targeted_reads = pfm[pfm["is_targeted"]]["num_reads"].sum()
    total_targeted_umis = pfm[pfm["is_targeted"]]["num_umis"].sum()
    out["multi_cdna_pcr_dupe_reads_frac_on_target"] = robust_divide(int(total_targeted_reads) - int(total_targeted_umis), int(total_targeted_reads))
    out.update(gene_counts(pfm))
    q = pfm[pfm["num_umis_cells"] >= MIN_UMIS]
    out["q_feature"] = q["feature_idx"].to_numpy().astype(np.uint32)
    out["q_value"] = q["mean_reads_per_umi_cells_log10"].to_numpy().astype(np.float64)
    out["q_label"] = q["is_targeted"].to_numpy().astype(np.uint8)
    return out, pfm


# ---- 3. the mixture fit -------------------------------------------------------------------------------------------------------------
def _wlp(x, w, mu, pc):
    y = x[:, None] * pc - mu[None, :] * pc
    return -0.5 * (np.log(2 * np.pi) + y * y) + np.log(pc) + np.log(w)[None, :]


def em_tied(x, w, mu, prec, max_iter=100, tol=1e-3, reg=1e-6):
    """-> weights, means, precision, sum of score_samples, weighted log probabilities, iterations, last |change|"""
    w = np.array(w, float)
    mu = np.array(mu, float)
    pc = math.sqrt(prec)
    lb = -np.inf
    it, change = 0, np.inf
    for it in range(1, max_iter + 1):
        prev = lb
        a = _wlp(x, w, mu, pc)
        lpn = logsumexp(a, axis=1)
        r = np.exp(a - lpn[:, None])
        nk = r.sum(0) + 10 * np.finfo(float).eps
        mu = (r.T @ x) / nk
        cov = (x @ x - (nk * mu) @ mu) / nk.sum() + reg
        w = nk / nk.sum()
        w = w / w.sum()
        pc = 1.0 / math.sqrt(cov)
        lb = lpn.mean()
        change = abs(lb - prev)
        if change < tol:
            break
    a = _wlp(x, w, mu, pc)
    return w, mu, pc * pc, logsumexp(a, axis=1).sum(), a, it, change


def initial_values(labels, values):
    """weights, label medians, the tied precision, the 5152 pairs of starting means (fit_2comp_gmm :36-65)"""
    labels = np.asarray(labels).astype(bool)
    nt, no = labels.sum(), (~labels).sum()
    iw = [nt / float(nt + no), no / float(nt + no)]
    im = [np.median(values[labels]), np.median(values[~labels])]
    sd_off = max(scipy.stats.iqr(values[~labels]) / 1.35, 1e-2)
    pairs = [im]
    grid = np.linspace(0, np.nanmax(values), RPU_NUM_TRIES + 1)
    for a in grid:
        for b in grid:
            if a < b:
                continue
            pairs.append([a, b])
    return iw, np.array(pairs, float), 1.0 / math.pow(sd_off, 2)


def fit(labels, values, starts=None):
    """fit_2comp_gmm(covariance_type=TIED).  starts: the starts to run (default all) -> dict with the seven RpuFitParams, the winner,
    per start lk / iterations / last change, the posterior of the high component"""
    values = np.asarray(values, float)
    iw, pairs, prec0 = initial_values(labels, values)
    assert len(pairs) == N_STARTS
    idx = range(len(pairs)) if starts is None else starts
    lks, its, changes = np.full(len(pairs), np.nan), np.zeros(len(pairs), np.uint32), np.full(len(pairs), np.nan)
    best, max_lk, winner = None, float("-inf"), -1
    for s in idx:
        w, mu, prec, lk, a, it, ch = em_tied(values, iw, pairs[s], prec0)
        lks[s], its[s], changes[s] = lk, it, ch
        if lk > max_lk:
            best, max_lk, winner = (w, mu, prec, a), lk, s
    w, mu, prec, a = best
    post = np.exp(a - logsumexp(a, axis=1)[:, None])
    hi, lo = int(np.argmax(mu)), int(np.argmin(mu))
    in_hi, in_lo = post[:, hi] > 0.5, post[:, lo] >= 0.5
    thr = np.min(values[in_hi]) if in_hi.sum() > 0 and in_lo.sum() > 0 else np.nan
    return dict(log_rpu_threshold=float(thr), mu_high=float(mu[hi]), mu_low=float(mu[lo]), sd_high=float(prec), sd_low=float(prec),
                alpha_high=float(w[hi]), alpha_low=float(w[lo]), winner=winner, max_lk=float(max_lk), lks=lks, its=its, changes=changes,
                post_high=post[:, hi])


def class_stats(labels, calls):
    labels = np.asarray(labels).astype(bool)
    return dict(n_targeted_enriched=float((labels & calls).sum()), n_targeted_not_enriched=float((labels & ~calls).sum()),
                n_offtgt_enriched=float((~labels & calls).sum()), n_offtgt_not_enriched=float((~labels & ~calls).sum()))


def fit_enrichments(labels, values, starts=None):
    """fit_enrichments(..., method=BOTH_TIED) (gmm.py:116-183): the seven parameters and the four class counts, NaN where the
    reference has NaN; `fitted` says whether the mixture ran"""
    labels = np.asarray(labels).astype(bool)
    values = np.asarray(values, float)
    nt = int(labels.sum())
    no = labels.shape[0] - nt
    nan = float("nan")
    out = {k: nan for k in FIT_KEYS + CLASS_KEYS}
    out["fitted"], out["winner"] = False, -1
    if nt == 0 and no == 0:
        pass
    elif no == 0:
        out["log_rpu_threshold"] = 0.0
        out.update(class_stats(labels, values >= 0.0))
    elif max(no, nt) < MIN_OFFTARGET_GENES or min(nt, no) == 0:
        pass
    else:
        f = fit(labels, values, starts)
        out.update(f)
        out["fitted"] = True
        with np.errstate(invalid="ignore"):
            out.update(class_stats(labels, values >= f["log_rpu_threshold"]))
    return out


# ---- the stage's summary --------------------------------------------------------------------------------------------------------------
def enrichment_metrics(fe, stats, disable_rpu_enrichments):
    """get_enrichment_metrics (:60-217) without the per-feature column, is_spatial False: fe = fit_enrichments' dict"""
    m = {"log_rpu_threshold": fe["log_rpu_threshold"], "lrpu_fitted_mean_1": fe["mu_high"], "lrpu_fitted_mean_2": fe["mu_low"],
         "lrpu_fitted_sd_1": fe["sd_high"], "lrpu_fitted_sd_2": fe["sd_low"], "lrpu_fitted_weight_1": fe["alpha_high"],
         "lrpu_fitted_weight_2": fe["alpha_low"]}
    te, tn, oe, on = (fe[k] for k in CLASS_KEYS)
    m["frac_on_target_genes_enriched"] = robust_divide(te, te + tn)
    with np.errstate(all="ignore"):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            m["frac_off_target_genes_enriched"] = float(np.nanmin([robust_divide(oe, oe + te), robust_divide(oe, oe + on)]))
    m.update({"num_rpu_enriched_genes_on_target": te, "num_rpu_non_enriched_genes_on_target": tn,
              "num_rpu_enriched_genes_off_target": oe, "num_rpu_non_enriched_genes_off_target": on})
    thr = fe["log_rpu_threshold"]
    if not np.isnan(thr) and disable_rpu_enrichments:
        f_on, f_off = m["frac_on_target_genes_enriched"], m["frac_off_target_genes_enriched"]
        if np.isnan(f_on) or f_on < 0.5 or (not np.isnan(f_off) and f_off > 0.5):
            m = {k: float("nan") for k in m}
            thr = float("nan")
    m.update({k: v for k, v in stats.items() if k.startswith("num_genes_")})
    return m, thr


def targeted_metrics(num_umis, num_reads, num_umis_cells, num_reads_cells, is_targeted, is_gex, median_umis_per_cell_on_target,
                     median_genes_per_cell_on_target, num_cells, total_reads, targeted_frac, untargeted_frac, starts=None, fe=None):
    """join() (:305-385): the summary dict and the enriched_rpu column (NaN / 0 / 1 per GEX feature, in feature order).  fe: the
    result of fit_enrichments when the caller has it already (5152 fits take ~10 s here)"""
    stats, pfm = rpu_stats(num_umis, num_reads, num_umis_cells, num_reads_cells, is_targeted, is_gex)
    s = {"median_umis_per_cell_on_target": float(median_umis_per_cell_on_target),
         "median_genes_per_cell_on_target": float(median_genes_per_cell_on_target),
         "total_targeted_reads_per_filtered_bc": robust_divide(float(targeted_frac) * total_reads, num_cells),
         "multi_frac_conf_transcriptomic_reads_on_target": targeted_frac,
         "multi_frac_conf_transcriptomic_reads_off_target": untargeted_frac}
    s.update({k: v for k, v in stats.items() if not k.startswith("q_") and not k.startswith("num_genes_")})
    key = s["mean_reads_per_umi_per_gene_cells_on_target"]
    disable = bool(np.isnan(key) or key < MIN_RPU_THRESHOLD)
    if fe is None:
        fe = fit_enrichments(stats["q_label"], stats["q_value"], starts)
    m, thr = enrichment_metrics(fe, stats, disable)
    s.update(m)
    col = np.full(len(pfm), np.nan)
    if not np.isnan(thr):
        with np.errstate(invalid="ignore"):
            col = (pfm["mean_reads_per_umi_cells_log10"].to_numpy() > thr).astype(np.float64)
    return s, col
