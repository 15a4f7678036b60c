"""The numpy restatement of the marginal caller (tests/marginal_calls_numpy.py), in cell order and in histogram order, against
tests/golden/marginal_calls_reference.npz (no GPU).

The golden file was recorded by scripts/make_marginal_calls_golden.py from the reference's own call_presence_with_gmm_ab and
TagAssigner.identify_contaminant_tags under scikit-learn 1.7.2 (the version is in the file).  The recorder rejected every fixture
whose stopping difference lies within 1e-9 of 1e-3 or whose Lloyd midpoints or decision boundary lie within 1e-9 of a data value, so
calls, winner, iteration count, umi_threshold_observed and the contaminant flags are asserted EQUAL here; weights, means and the tied
covariance must lie within the movement the recorder measured (absolute, per kind, the maximum over all fixtures): cell order
within `movement_reference` of the reference, histogram order within `movement_forms` of cell order and so within their sum of
the reference.  `movement` is the larger of the two: what a change of the summation order does to this arithmetic, and the unit of
the device's bound."""
import os

import numpy as np
import pytest

import marginal_calls_numpy as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "marginal_calls_reference.npz")
_CACHE = {}


def golden():
    if "g" not in _CACHE:
        with np.load(GOLDEN) as z:
            _CACHE["g"] = {k: z[k] for k in z.files}
    return _CACHE["g"]


def fixture_names():
    return [str(n) for n in golden()["names"]]


def fixture_row(i):
    """-> (V, cols, vals, umi_threshold, dense counts)"""
    g = golden()
    V, lo, hi = int(g["V"][i]), int(g["row_ptr"][i]), int(g["row_ptr"][i + 1])
    cols, vals = g["cols"][lo:hi], g["vals"][lo:hi]
    dense = np.zeros(V, np.int64)
    dense[cols] = vals
    return V, cols, vals, int(g["umi_threshold"][i]), dense


def restated(i):
    """the histogram-order restatement of fixture i, computed once per session and shared with the GPU tests"""
    key = ("hist", i)
    if key not in _CACHE:
        V, cols, vals, thr, _ = fixture_row(i)
        _CACHE[key] = R.fit_histogram(V, cols, vals, thr)
    return _CACHE[key]


def reference_calls(i):
    g = golden()
    return g["calls"][int(g["call_ptr"][i]):int(g["call_ptr"][i + 1])]


def parameters(res):
    return np.array([res["weight_low"], res["weight_high"], res["mean_low"], res["mean_high"], res["covariance"]])


def distances(a, b):
    """max |a - b| over the weights, over the means, and of the covariance"""
    d = np.abs(np.asarray(a) - np.asarray(b))
    return np.array([d[:2].max(), d[2:4].max(), d[4]])


def check_against_golden(i, res, called_cols, bound):
    """integers equal, parameters within `bound` (weights, means, covariance; absolute); -> the three distances"""
    g = golden()
    assert np.array_equal(called_cols, reference_calls(i))
    assert bool(res["fitted"]) == bool(g["fitted"][i])
    if not res["fitted"]:
        return np.zeros(3)
    _, cols, vals, thr, dense = fixture_row(i)
    want_thr = int(dense[reference_calls(i)].min()) if len(reference_calls(i)) else -1
    assert res["n_iter"] == int(g["n_iter"][i]) and res["umi_threshold_observed"] == want_thr and res["cells_assigned"] == len(reference_calls(i))
    d = distances(parameters(res), np.concatenate((g["weights"][i], g["means"][i], [g["covariance"][i]])))
    assert np.all(d <= bound), (fixture_names()[i], d, bound)
    return d


def test_golden_file_is_what_the_tests_assume():
    g = golden()
    assert str(g["sklearn_version"]) == R.SKLEARN_VERSION == "1.7.2"
    assert set(g["V"].tolist()) == {2, 3, 65, 257, 5000} and 20 <= len(g["names"]) <= 60
    assert os.path.getsize(GOLDEN) < 1 << 20
    assert np.all(g["movement"] > 0) and np.all(g["movement"] < 1e-10) and np.array_equal(g["movement"], np.maximum(g["movement_reference"], g["movement_forms"]))
    assert g["landings"].min() > 0 and g["first_kinds"].min() > 0
    u, _ = R.seed_draws(300)
    assert g["draws"].tobytes() == u.ravel().tobytes() and list(g["draw_order"][:3]) == ["choice", "uniform", "uniform"]
    nd = [len(restated(i).get("values", [])) for i in range(len(g["names"]))]
    assert any(64 < n <= 256 for n in nd) and any(n > 256 for n in nd) and any(n == 1 for n in nd)


@pytest.mark.parametrize("i", range(len(np.load(GOLDEN)["names"])))
def test_both_forms_equal_the_reference(i):
    V, cols, vals, thr, dense = fixture_row(i)
    cell = R.fit_dense(dense, thr)
    hist = restated(i)
    g = golden()
    # cell order against the reference, histogram order against cell order: the two distances the recorder measured; histogram order
    # against the reference: at most their sum
    check_against_golden(i, cell, np.flatnonzero(cell["calls"]), g["movement_reference"])
    check_against_golden(i, hist, cols[hist["calls"]], g["movement_reference"] + g["movement_forms"])
    if cell["fitted"]:
        assert cell["winner"] == hist["winner"] and np.array_equal(cell["n_iters"], hist["n_iters"])
        assert np.all(distances(parameters(cell), parameters(hist)) <= g["movement_forms"])


def test_hand_cases():
    # V = 2: one zero and one count; the two values are the two clusters
    r = R.fit_histogram(2, [1], [3], 1)
    assert r["fitted"] and list(r["calls"]) == [True] and r["umi_threshold_observed"] == 3
    assert abs(r["mean_low"]) < 1e-12 and abs(r["mean_high"] - np.log10(4)) < 1e-12 and abs(r["weight_low"] - 0.5) < 1e-12
    assert not R.fit_histogram(2, [1], [3], 4)["calls"].any()                    # the threshold alone keeps the cell out
    d = R.fit_dense([0, 3], 1)
    assert list(d["calls"]) == [False, True] and d["n_iter"] == r["n_iter"]
    # an all-zero row, and a single cell: not fitted, no calls
    for res in (R.fit_dense([0, 0, 0]), R.fit_histogram(3, [], []), R.fit_dense([5]), R.fit_histogram(1, [0], [5])):
        assert not res["fitted"] and not res["calls"].any() and res["umi_threshold_observed"] == -1
    # one distinct value: fitted; the second cluster is empty (mean 0, weight of a few eps) and every cell is called when the value
    # meets the threshold
    for thr, want in ((1, True), (5, True), (6, False)):
        r = R.fit_histogram(4, [0, 1, 2, 3], [5, 5, 5, 5], thr)
        d = R.fit_dense([5, 5, 5, 5], thr)
        assert r["fitted"] and d["fitted"] and list(r["calls"]) == [want] * 4 == list(d["calls"])
        assert r["mean_low"] == 0.0 and r["weight_low"] < 1e-14 and abs(r["mean_high"] - np.log10(6)) < 1e-12 and abs(r["covariance"] - 1e-6) < 1e-12
    # one distinct non-zero value among zeros: the ordinary two-cluster case
    r = R.fit_histogram(6, [1, 4], [7, 7], 3)
    assert list(r["calls"]) == [True, True] and list(r["values"]) == [0, 7] and list(r["multiplicities"]) == [4, 2]


def test_contaminant_rule():
    g = golden()
    flags, src = R.identify_contaminants(g["cont_counts"], g["cont_order"])
    assert np.array_equal(flags, g["cont_flags"])
    for t in range(len(flags)):
        assert src[t] == [int(x) for x in g["cont_sources"][t] if x >= 0]
    # a NaN correlation is skipped: a constant tag next to a copy of another
    c = np.array([[900, 0, 900, 0], [5, 5, 5, 5], [450, 0, 450, 1]], np.int64) * 3
    flags, src = R.identify_contaminants(c, [0, 1, 2], min_counts=10)
    assert list(flags) == [0, 1, 1] and src == [[], [], [0]]      # tag 1: 50-fold below; tag 2 follows tag 0; no source through the NaN


def test_snr():
    assert R.umi_interval_snr([0, 0, 1, 2, 50, 60, 70], 50) == float(np.round(np.log10(55 + 1) - np.log10(1.25 + 1), 3))
    assert R.umi_interval_snr([5, 6], 1) == float(np.round(np.log10(5.25 + 1), 3))
