"""CPU checks that pin tests/umap_numpy.py, the restatement RUN_UMAP on the device is held to, and the host function crgpu_umap_ab, to
yardsticks that are independent of both: scipy 1.15.3 (curve_fit for the curve, scipy.sparse for the fuzzy union) and mpmath (psum at
the sigma a search ended on).  tests/golden/umap_reference.npz (scripts/make_umap_golden.py) must be what the restatement gives today.
No GPU: the device is compared with the file and the restatement in tests/test_gpu_umap.py."""
import os

import numpy as np
import pytest

import umap_numpy as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "umap_reference.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def test_the_curve_fit_agrees_with_scipy(golden):
    """umap_ab of the restatement and crgpu_umap_ab of the library against scipy.optimize.curve_fit at ftol = xtol = gtol = 1e-14 (run
    by the maker): within 16 times the distance between scipy's answers from the starts (1, 1) and (2, 0.5), floored at 1e-12
    relative.  For orientation: scipy's defaults give a = 0.99218, b = 1.11225 at (0.3, 1)."""
    from cellranger_amd import build, engine

    build.build()
    assert np.array_equal(golden["ab_cases"], np.array(R.AB_CASES))
    assert abs(golden["ab_scipy"][0][0] - 0.99218) < 1e-5 and abs(golden["ab_scipy"][0][1] - 1.11225) < 1e-5
    for (min_dist, spread), want, bound in zip(R.AB_CASES, golden["ab_scipy"], golden["ab_bound"]):
        assert (bound >= 1e-12 * np.abs(want)).all()
        for who, got in (("restatement", R.umap_ab(min_dist, spread)), ("library", engine.umap_ab(min_dist, spread))):
            off = np.abs(np.array(got) - want)
            print("%s (%g, %g): a %.15g b %.15g, off by %.3g, %.3g of the bound" % (who, min_dist, spread, got[0], got[1], *(off / bound)))
            assert (off <= bound).all(), (who, min_dist, spread)
    assert engine.umap_ab() == engine.umap_ab(0.3, 1.0)


@pytest.mark.parametrize("name", list(R.FIXTURES))
def test_golden_file_is_the_restatement(golden, name):
    g = R.prepared(name)
    for key in ("rho", "sigma", "steps", "indptr", "indices", "values"):
        assert g[key].dtype == golden["%s_%s" % (name, key)].dtype and g[key].tobytes() == golden["%s_%s" % (name, key)].tobytes(), key
    h = np.abs(g["decisions"])
    assert not (np.abs(h - R.TOL) < 1e-9).any() and not (np.abs(g["union_values"] - g["threshold"]) < 1e-9 * g["threshold"]).any()
    assert os.path.getsize(GOLDEN) < 512 * 1024


@pytest.mark.parametrize("name", list(R.FIXTURES))
def test_psum_at_sigma_in_mpmath(name):
    """Every row's psum at the mid its search ended on, in 50 digits, is within 1e-5 of log2(k + 1), or the row ended at 64 steps, or the
    floor applied; rho is the first distance > 0 and the constructed rows are what they were built to be."""
    import mpmath

    mpmath.mp.dps = 50
    g = R.prepared(name)
    d, k = g["nn_distances"], g["k"]
    target = mpmath.log(k + 1, 2)
    checked = 0
    for i in range(len(d)):
        pos = d[i][d[i] > 0]
        assert g["rho"][i] == (pos[0] if len(pos) else 0.0)
        if g["steps"][i] == R.MAX_STEPS or g["floored"][i]:
            continue
        assert g["sigma"][i] == g["mid"][i]
        psum = mpmath.mpf(0)
        for v in d[i]:
            x = mpmath.mpf(float(v)) - mpmath.mpf(float(g["rho"][i]))
            psum += mpmath.exp(-(x / mpmath.mpf(float(g["sigma"][i])))) if x > 0 else 1
        assert abs(psum - target) < mpmath.mpf(R.TOL) + mpmath.mpf(10) ** -12, (i, float(psum - target))
        checked += 1
    ended, floored = int((g["steps"] == R.MAX_STEPS).sum()), int(g["floored"].sum())
    print("%s: %d rows checked, %d ended at 64 steps, %d at the floor" % (name, checked, ended, floored))
    assert checked + len(set(np.flatnonzero(g["steps"] == R.MAX_STEPS)) | set(np.flatnonzero(g["floored"]))) == len(d)
    if name == "duplicates":      # the k + 2 equal rows: all distances 0, rho 0, 64 steps, the all-distances floor, the entry (i, i)
        block = np.arange(17)
        assert not d[block].any() and not g["rho"][block].any() and (g["steps"][block] == 64).all() and g["floored"][block].all()
        total = R.ordered_sum(np.cumsum(d, axis=1)[:, -1])
        assert (g["sigma"][block] == R.FLOOR * (total / (120.0 * 16.0))).all()
        rows = np.repeat(np.arange(120), np.diff(g["indptr"]))
        assert (rows == g["indices"]).sum() >= 1
    if name == "hub":
        assert (np.diff(g["indptr"])[57] == 129) and all(57 in g["nn_indices"][i] for i in range(130) if i != 57)
    if name == "chain":
        assert g["k"] == 1 and (g["nn_indices"][:-1, 0] == np.arange(1, 24)).all() and (g["steps"] == 1).all()
    if name == "zero_variance":
        assert not g["rows"][7].any() and g["floored"][7] and g["steps"][7] == 64
    if name == "three_groups":
        assert g["k"] == 29 and ended == 0 and floored == 0


@pytest.mark.parametrize("name", list(R.FIXTURES))
def test_the_union_is_scipys_and_twins_carry_equal_bits(name):
    import scipy.sparse as sp

    g = R.prepared(name)
    n, k = g["nn_indices"].shape
    A = sp.csr_matrix((g["memb"].reshape(-1), (np.repeat(np.arange(n), k), g["nn_indices"].reshape(-1))), shape=(n, n))
    want = (A + A.T - A.multiply(A.T)).toarray()
    mine = np.zeros((n, n))
    mine[g["union_keys"] // n, g["union_keys"] % n] = g["union_values"]
    assert mine.tobytes() == want.tobytes()
    kept = np.zeros((n, n))
    kept[np.repeat(np.arange(n), np.diff(g["indptr"])), g["indices"]] = g["values"]
    assert kept.tobytes() == np.where(want >= want.max() / g["n_epochs"], want, 0.0).tobytes()
    assert kept.tobytes() == np.ascontiguousarray(kept.T).tobytes() and g["wmax"] == 1.0
    for i in range(n):      # ascending columns
        assert (np.diff(g["indices"][g["indptr"][i]:g["indptr"][i + 1]]) > 0).all()


def test_metric_input_and_the_start():
    from cellranger_amd import engine

    x = R.FIXTURES["zero_variance"].x
    for metric in R.METRICS:
        rows, angular = R.metric_input(x, metric)
        theirs, flag = engine.umap_metric_input(x, metric)
        assert rows.tobytes() == theirs.tobytes() and angular == flag == (metric != "euclidean")
    rows, _ = R.metric_input(x, "correlation")
    assert not rows[7].any()
    live = np.delete(np.arange(len(x)), 7)
    d2 = ((rows[live][:, None, :] - rows[live][None]) ** 2).sum(axis=2)
    assert np.abs(0.5 * d2 - (1.0 - np.corrcoef(x[live]))).max() < 1e-12
    cos, _ = R.metric_input(x, "cosine")
    assert np.abs((cos[live] ** 2).sum(axis=1) - 1.0).max() < 1e-12 and not np.allclose(cos[live], rows[live])
    assert R.metric_input(x, "pearson")[0].tobytes() == rows.tobytes()
    with pytest.raises(ValueError):
        engine.umap_metric_input(x, "manhattan")
    y = np.array([[1.0, 5.0, 2.0], [3.0, 5.0, -2.0], [2.0, 5.0, 0.0]])
    want = np.array([[0.0, 0.0, 10.0], [10.0, 0.0, 0.0], [5.0, 0.0, 5.0]])
    assert np.array_equal(R.rescale(y), want) and np.array_equal(engine.umap_rescale(y), want)
    assert R.stage_neighbors(2) == (1, True) and R.stage_neighbors(3) == (2, False) and R.stage_neighbors(500) == (30, False)
    assert R.default_epochs(10000) == 500 and R.default_epochs(10001) == 200
    assert (engine.get_umap_name("Gene Expression", 2), engine.get_umap_key("Gene Expression", 2)) == ("gene_expression_2-d", "2")
    assert (engine.get_umap_name("Antibody Capture", 3), engine.get_umap_key("Antibody Capture", 3)) == ("antibody_capture_3-d", "antibody_capture_3")


@pytest.mark.parametrize("rate", [1, 5, 8])
def test_the_schedule(rate):
    """Over n_epochs an entry of weight w is active floor(n_epochs * w / wmax) times, within 1; n_neg never exceeds 2 rate - 1 <= 15 (the
    restatement asserts 15 itself), and the samples of an entry come to rate per activation in the long run."""
    indptr, indices, values, Y = R.synthetic_graph(65, 2, 7)
    n_epochs = 150
    eons, eonns = R.schedule(values, 1.0, rate)
    count, negs, worst = np.zeros(len(values), np.int64), np.zeros(len(values), np.int64), 0
    for n in range(n_epochs):
        _, eons, eonns, info = R.epoch(indptr, indices, values, Y, eons, eonns, n, n_epochs, 1.0, 1.0, 3, rate=rate, wmax=1.0)
        count[info["active"]] += 1
        negs[info["active"]] += info["n_neg"]
        worst = max(worst, int(info["n_neg"].max()) if len(info["n_neg"]) else 0)
    want = np.floor(n_epochs * values / 1.0)
    assert values.max() == 1.0 and (np.abs(count - want) <= 1).all() and count.max() >= n_epochs - 1
    assert worst <= 2 * rate - 1 <= R.MAX_NEG
    # After an entry's last activation, at epoch n: eonns = (negs + 1) epns lies in (n - epns, n], so negs + 1 is in (n / epns - 1,
    # n / epns]; eons = (count + 1) eps with eons - eps <= n < eons + 1, so n / epns = rate n / eps is in [rate count, rate count + 2 rate).
    # Together: rate count - 2 < negs <= rate count + 2 rate - 1 (one more on either side for the roundings of the two states)
    seen = count > 0
    diff = negs[seen] - rate * count[seen]
    assert seen.sum() > 100 and (diff >= -2).all() and (diff <= 2 * rate).all()


def test_an_epoch_is_a_pure_function_and_two_calls_equal_one():
    g = R.prepared("hub")
    a, b = R.umap_ab()
    csr = (g["indptr"], g["indices"], g["values"])
    one = R.run(*csr, g["y0"], 0, 12, 200, a, b, 5)
    first = R.run(*csr, g["y0"], 0, 7, 200, a, b, 5)
    two = R.run(*csr, first[0], 7, 5, 200, a, b, 5, eons=first[1], eonns=first[2])
    assert all(one[i].tobytes() == two[i].tobytes() for i in range(3))
    other = R.run(*csr, g["y0"], 0, 12, 200, a, b, 6)
    assert other[0].tobytes() != one[0].tobytes() and other[1].tobytes() == one[1].tobytes()      # the seed moves the samples, not the schedule
    words = R.philox_words(5, 3, 8)
    assert words.dtype == np.uint64 and np.array_equal(words, np.random.Philox(counter=[0, 3, 0, 0], key=[5, 0]).random_raw(8))
