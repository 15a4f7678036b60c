"""The numpy restatement tests/matrix_summary_numpy.py of the filtered-matrix summary (no GPU): against the reference's recorded
sum_masked / count_ge_masked outputs (tests/golden/matrix_summary_reference.npz, written by scripts/make_matrix_summary_golden.py),
against numbers worked out by hand on a 6 x 8 matrix, numpy's percentile rule from two order statistics, and the two checks of the
standard deviation:
  (a) exact: Python integers give N = n sum(x^2) - (sum x)^2 without rounding; math.sqrt(Fraction(N, n n)) rounds the quotient once
      (0.5 ulp, halved by the root) and the root once (0.5 ulp).  A f64 evaluation rounds N, n^2 (for n >= 2^26), the quotient and
      the root: at most (0.5 + 0.5 + 0.5) / 2 + 0.5 = 1.25 ulp of its own, so 4 ulp between the two is generous and fixed.
  (b) np.std: one rounding per difference and per square, a blocked pairwise sum of about 8 + log2(n / 128) roundings, half of that
      after the root: well under 32 * 2^-53 relative for n <= 2^20 on inputs with cv >= 1e-3; 64 * 2^-53 is asserted."""
import math
import os
from fractions import Fraction

import numpy as np
import pytest

import matrix_summary_numpy as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "matrix_summary_reference.npz")


def ulp_distance(a, b):
    a, b = np.float64(a).view(np.int64), np.float64(b).view(np.int64)
    return abs(int(a) - int(b))


def f64_std(n, s, q):
    """the evaluation crgpu_matrix_summary_stats makes: N exact, then f64"""
    return math.sqrt(float(n * q - s * s) / (float(n) * float(n)))


# ---- the reference's recorded outputs ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.golden_fixtures()))
def test_restatement_equals_the_references_masked_sums(name):
    g, fx = np.load(GOLDEN), R.golden_fixtures()[name]
    V, cells = len(fx["indptr"]) - 1, fx["cells"].astype(np.int64)
    args = (fx["indptr"], fx["indices"].astype(np.int64), fx["data"].astype(np.int64), fx["n_features"])
    listed = np.zeros(V, bool)
    listed[cells] = True
    s = R.run(fx)
    for k in range(fx["n_classes"]):
        rows = fx["feature_class"] == k
        own_cells = ((fx["cell_class_mask"] >> np.uint32(k)) & 1).astype(bool)
        own = np.zeros(V, bool)
        own[cells[own_cells]] = True
        for vname, cols in (("own", own), ("union", listed), ("all", np.ones(V, bool))):
            key = "%s_c%d_%s" % (name, k, vname)
            for axis, tag in ((0, "0"), (1, "1"), (None, "n")):
                assert np.array_equal(np.asarray(R.sum_masked(*args, rows, cols, axis)).astype(np.int64), g[key + "_sum_" + tag]), (key, axis)
                for thr in (1, 2):
                    got = np.asarray(R.count_ge_masked(*args, rows, cols, thr, axis)).astype(np.int64)
                    assert np.array_equal(got, g["%s_ge%d_%s" % (key, thr, tag)]), (key, thr, axis)
        # ... and the summary's fields are those outputs
        c, key = s["classes"][k], "%s_c%d_" % (name, k)
        assert np.array_equal(s["counts_per_feature"][rows].astype(np.int64), g[key + "own_sum_1"])
        assert np.array_equal(s["cells_ge2_per_feature"][rows].astype(np.int64), g[key + "own_ge2_1"])
        assert np.array_equal(s["counts_per_cell"][k, own_cells].astype(np.int64), g[key + "own_sum_0"])
        assert np.array_equal(s["genes_per_cell"][k, own_cells].astype(np.int64), g[key + "own_ge1_0"])
        assert not s["counts_per_cell"][k, ~own_cells].any() and not s["genes_per_cell"][k, ~own_cells].any()
        assert c["raw_total_counts"] == int(g[key + "all_sum_n"]) and c["union_total_counts"] == int(g[key + "union_sum_n"])
        assert c["union_nnz"] == int(g[key + "union_ge1_n"])
        assert c["cells_total_counts"] == int(g[key + "own_sum_n"]) and c["cells_nnz"] == int(g[key + "own_ge1_n"])
        assert c["genes_detected"] == int(np.count_nonzero(g[key + "own_sum_1"]))
        # top_n of the reference (argpartition + argsort) on the recorded row sums: the same multiset of values, the same ids above a tie
        for field, rec in (("top_counts", g[key + "own_sum_1"]), ("top_cells", g[key + "own_ge2_1"])):
            n = c["n_top"]
            idx = np.argpartition(rec, -n)[-n:]
            idx = idx[np.argsort(rec[idx])]
            assert sorted(c[field + "_value"]) == sorted(int(v) for v in rec[idx])
            feats = np.flatnonzero(rows)
            boundary = min(c[field + "_value"])
            untied = [(int(feats[i]), int(rec[i])) for i in idx if rec[i] > boundary or np.sum(rec == boundary) == np.sum(rec[idx] == boundary)]
            assert set(untied) <= set(zip(c[field + "_feature"], c[field + "_value"]))


# ---- hand cases --------------------------------------------------------------------------------------------------------------------
def test_hand_matrix():
    fx = R.hand_matrix()
    s = R.run(fx)
    # class 0 = features 0 1 2 over the cells 1 and 3; class 1 = features 3 4 over the cells 3 and 6; feature 5 in no class
    assert s["counts_per_feature"].tolist() == [5 + 2, 1, 4, 1 + 2, 6 + 2, 0]
    assert s["cells_ge2_per_feature"].tolist() == [2, 0, 1, 1, 2, 0]      # (0, 1) = 5 and (0, 3) = 2 count, (1, 1) = 1 does not
    c0, c1 = s["classes"]
    assert (c0["n_features_class"], c0["n_cells"], c1["n_features_class"], c1["n_cells"]) == (3, 2, 2, 2)
    assert c0["raw_total_counts"] == 3 + 5 + 1 + 2 + 4 + 8 + 1 + 11 and c1["raw_total_counts"] == 7 + 1 + 6 + 1 + 2 + 2
    assert (c0["union_total_counts"], c0["union_nnz"]) == (5 + 1 + 2 + 4 + 11, 5) and (c1["union_total_counts"], c1["union_nnz"]) == (7 + 1 + 6 + 2 + 2, 5)
    assert (c0["cells_total_counts"], c0["cells_nnz"], c0["genes_detected"]) == (12, 4, 3)
    assert (c1["cells_total_counts"], c1["cells_nnz"], c1["genes_detected"]) == (11, 4, 2)
    assert s["counts_per_cell"].tolist() == [[6, 6, 0], [0, 7, 4]] and s["genes_per_cell"].tolist() == [[2, 2, 0], [0, 2, 2]]
    assert (c0["counts_sum"], c0["counts_sumsq_lo"], c0["genes_sum"], c0["genes_sumsq_lo"]) == (12, 72, 4, 8)
    assert (c1["counts_sum"], c1["counts_sumsq_lo"], c1["counts_sumsq_hi"]) == (11, 65, 0)
    assert c0["counts_q"] == [6, 6, 6, 6, 6, 6] and c1["counts_q"] == [4, 7, 4, 7, 4, 7]
    assert (c0["n_top"], c0["top_counts_feature"], c0["top_counts_value"]) == (3, [0, 2, 1], [7, 4, 1])
    assert (c0["top_cells_feature"], c0["top_cells_value"]) == ([0, 2, 1], [2, 1, 0])
    assert (c1["n_top"], c1["top_counts_feature"], c1["top_counts_value"]) == (2, [4, 3], [8, 3])
    assert (c0["reads_cells"], c1["reads_cells"], s["reads_union"], s["reads_all"]) == (70, 90, 120, 164)
    f1 = R.class_floats(c1, c1["reads_cells"], s["reads_all"])
    assert (f1["counts_mean"], f1["counts_median"], f1["counts_iqr"], f1["counts_std"]) == (5.5, 5.5, 1.5, 1.5)
    assert f1["counts_cv"] == 1.5 / 5.5 and f1["genes_cv"] == 0.0 and f1["density"] == 1.0 and f1["cum_frac"] == 11 / 19
    assert f1["dupe_frac"] == 1 - 11 / 90 and f1["reads_per_cell"] == 45.0 and f1["reads_cum_frac"] == 90 / 164


def test_an_empty_class_and_no_cells():
    fx = R.hand_matrix()
    s = R.run(fx, cell_class_mask=np.array([1, 1, 0], np.uint32))      # no cell of class 1; cell 6 is listed and of no class
    c1 = s["classes"][1]
    assert (c1["n_cells"], c1["cells_total_counts"], c1["cells_nnz"], c1["genes_detected"], c1["counts_sum"]) == (0, 0, 0, 0, 0)
    assert c1["raw_total_counts"] == 19 and c1["union_total_counts"] == 18 and c1["counts_q"] == [0] * 6
    assert c1["top_counts_feature"] == [3, 4] and c1["top_counts_value"] == [0, 0]      # ties: by feature index
    f = R.class_floats(c1, 0, s["reads_all"])
    assert all(math.isnan(f[k]) for k in ("counts_mean", "counts_median", "counts_cv", "counts_iqr", "density", "dupe_frac", "reads_per_cell"))
    assert f["cum_frac"] == 0.0 and f["reads_cum_frac"] == 0.0
    none = R.summary(fx["indptr"], fx["indices"], fx["data"], 6, np.zeros(0, np.uint64), fx["feature_class"], 2, np.zeros(0, np.uint32), fx["reads"])
    assert not none["counts_per_feature"].any() and none["classes"][0]["raw_total_counts"] == 35 and none["reads_union"] == 0
    assert R.report(fx["indptr"], fx["indices"], fx["data"], 6, np.zeros(0, np.uint64), 0, "GRCh38", list("abcdef"), fx["feature_class"], 2) == {}


def test_report_of_the_hand_matrix():
    fx = R.hand_matrix()
    ids = ["G0", "G1", "G2", "G3", "G4", "G5"]
    d = R.report(fx["indptr"], fx["indices"], fx["data"], 6, fx["cells"], 1, "mm10", ids, fx["feature_class"], 2, fx["cell_class_mask"], fx["reads"],
                 total_reads=1000, conf_mapped_reads=800, recovered_cells=5)
    assert d["mm10_filtered_bcs_top_genes_with_reads"] == {"G4": 8, "G3": 3} and d["mm10_filtered_bcs_top_genes_with_unique_bcs"] == {"G4": 2, "G3": 1}
    assert d["mm10_filtered_bcs_total_unique_genes_detected"] == 2 and d["mm10_filtered_bcs_total_counts"] == 11
    assert d["mm10_filtered_bcs_median_counts"] == 5.5 and d["mm10_filtered_bcs_mean_unique_genes_detected"] == 2.0
    assert d["mm10_filtered_bcs_cum_frac"] == 11 / 19 and d["mm10_filtered_bcs_cdna_pcr_dupe_reads_frac"] == 1 - 11 / 90
    assert d["mm10_filtered_bcs_conf_mapped_barcoded_reads_cum_frac"] == 90 / 164
    assert d["filtered_bcs_transcriptome_union"] == 3 and d["reads_per_cell"] == 1000 / 3
    assert d["multi_filtered_bcs_difference_from_recovered_cells"] == -2 and d["multi_filtered_bcs_relative_difference_from_recovered_cells"] == -2 / 5
    assert d["multi_filtered_gene_bc_matrix_density"] == 10 / 15 and d["feature_reads_in_cells"] == 120 / 164
    assert d["multi_usable_reads"] == 120 and d["frac_feature_reads_usable"] == 0.12
    assert d["mm10_total_conf_mapped_deduped_barcoded_reads_per_filtered_bc"] == (23 + 18) / 3 and d["mm10_total_raw_reads_per_filtered_bc"] == 1000 / 3


# ---- the percentile rule and the standard deviation ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 8, 101])
def test_percentile_rule_equals_numpy(n):
    for seed in range(20):
        x = np.random.RandomState(1000 * n + seed).randint(0, [3, 1000, 2 ** 32][seed % 3], n).astype(np.int64)
        q = R.order_stats(x)
        med, p25, p75 = (R.lerp_percentile(n, i, q[2 * i - 2], q[2 * i - 1]) for i in (2, 1, 3))
        assert med == np.median(x) and p25 == np.percentile(x, 25) and p75 == np.percentile(x, 75)
        assert p75 - p25 == np.percentile(x, 75) - np.percentile(x, 25)
        assert float(R.moments(x)[0]) / n == np.mean(x)


STD_SIZES = [1, 2, 3, 7, 128, 129, 1000, 20000, 100003, 1 << 20]


@pytest.mark.parametrize("n", STD_SIZES)
def test_std_is_within_4_ulp_of_the_exact_value(n):
    for seed, hi in enumerate((2, 5000, 2 ** 32)):
        x = np.random.RandomState(77 * n + seed).randint(0, hi, n).astype(np.int64)
        s, q = R.moments(x)
        got, exact = f64_std(n, s, q), R.exact_std(x)
        print("n = %d, values < %d: %d ulp" % (n, hi, ulp_distance(got, exact)))
        assert ulp_distance(got, exact) <= 4


def test_std_with_a_square_of_n_that_rounds():
    """n >= 2^26: n^2 is not a f64; the moments are built without an array"""
    n = (1 << 27) + 12345
    a, b = 3, 40001      # n - 5 values a and 5 values b
    s, q = (n - 5) * a + 5 * b, (n - 5) * a * a + 5 * b * b
    exact = math.sqrt(Fraction(n * q - s * s, n * n))
    assert float(n) * float(n) != n * n
    assert ulp_distance(f64_std(n, s, q), exact) <= 4


@pytest.mark.parametrize("n", [n for n in STD_SIZES if n > 1])
def test_std_is_close_to_numpys(n):
    for seed, (lo, hi) in enumerate(((0, 5000), (1000, 1020), (0, 2 ** 32))):
        x = np.random.RandomState(99 * n + seed).randint(lo, hi, n).astype(np.int64)
        s, q = R.moments(x)
        got, ref = f64_std(n, s, q), float(np.std(x))
        if ref < 1e-3 * np.mean(x):
            continue
        print("n = %d: relative difference %.3g" % (n, abs(got - ref) / ref))
        assert abs(got - ref) <= 64 * 2.0 ** -53 * ref
