"""The sSeq restatement (tests/sseq_numpy.py) against cases worked out by hand, against exact arithmetic on the spot, and against
tests/golden/sseq_reference.npz (scripts/make_sseq_golden.py).  check_against_golden is the check the GPU test shares.

Hand case A, Poisson branch, 3 genes x 4 cells:
    x = [[1, 1, 1, 1], [2, 0, 2, 0], [1, 3, 1, 3]]      every column sums to 4: the median is 4, every size factor is 1, S = 4
    mean = [1, 1, 2], mean of squares = [1, 2, 5], var = [0, 1, 1]: gene 0 is not used
    phi_mm = max(0, (4 var - mean 4) / (mean^2 4)) = [-, 0, max(0, -4 / 16)] = 0: zeta_hat = 0, delta = 0 / 0, phi = [NaN, 0, 0]
    labels [1, 2, 1, 2]: s_a = s_b = 2 for both clusters.  Cluster 1: x_a = [2, 4, 2], x_b = [2, 0, 6].
    With phi = 0 and s_a = s_b the terms are proportional to the binomial coefficients C(T, i).
    gene 1: T = 4, observed i = 4, C = 1: the terms not above it are i = 0 and i = 4 (the mirrored term counts): p = 2 / 16
    gene 2: T = 8, observed i = 2, C = 28: i = 0, 1, 2, 6, 7, 8: p = (1 + 8 + 28) 2 / 256 = 74 / 256
    Benjamini-Hochberg over the two used genes: (2 / 2) 74 / 256, then min(that, (2 / 1) 2 / 16) = 1 / 4
    norm_mean_a = x_a / 2; log2_fold_change of gene 1 = log2(5 / 3) - log2(1 / 3) = log2(5)
    Cluster 2 mirrors cluster 1: the same p-values.
Hand case B, shrinkage, 3 genes x 4 cells:
    x = [[1, 1, 1, 1], [4, 0, 0, 0], [0, 4, 4, 4]]      every column sums to 5: size factors 1, S = 4
    gene 1: mean 1, mean of squares 4, var 3, phi_mm = (12 - 4) / 4 = 2;  gene 2: mean 3, mean of squares 12, var 3, phi_mm = (12 - 12) / 36 = 0
    zeta_hat = the 99.5th percentile of [0, 2] = 1.99; mean(phi_mm) = 1
    delta = ((1 + 1) / (G - 1 = 2)) / ((0.01^2 + 1.99^2) / (G - 2 = 1)) = 1 / 3.9602
    phi = [NaN, 2 - 0.01 delta, 1.99 delta]
Benjamini-Hochberg with ties: p = [0.01, 0.04, 0.04, 0.03, 0.5], n = 5: ranks 1, 3, 4, 2, 5; n p / rank = 0.05, 0.0667, 0.05, 0.075, 0.5; the
    running minimum from the largest p downwards gives 0.05 for the four small ones (the two equal p get equal q) and 0.5."""
import os

import numpy as np
import pytest

import sseq_numpy as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN = 16.0      # the project's standing margin over the reference's own movement
_GOLDEN = []
EQUAL = ("use_g", "n_used", "size_factors", "sums_in", "sums_out", "below_median", "n_exact", "n_asymptotic")
# quantity -> (dev_<q> of the golden file, the floor of the relative error's denominator)
FLOATS = dict(mean_g=("mean_g", 0.0), var_g=("var_g", 0.0), phi_mm_g=("phi_g", 0.0), phi_g=("phi_g", 0.0), zeta_hat=("zeta_hat", 0.0), delta=("delta", 0.0),
              norm_mean_in=("norm_mean", 0.0), norm_mean_out=("norm_mean", 0.0), s_a=("norm_mean", 0.0), s_b=("norm_mean", 0.0),
              log2_fold_change=("log2_fold_change", 1.0))


def golden():
    if not _GOLDEN:
        _GOLDEN.append(np.load(os.path.join(ROOT, "tests", "golden", "sseq_reference.npz")))
    return _GOLDEN[0]


def fixture(name):
    g = golden()
    x, labels, K = R.fixture(name, int(g[name + "/bump"]))
    assert int(x.sum()) == int(g[name + "/x_sum"]) and np.array_equal(labels, g[name + "/labels"]), "the fixture is not the recorded one"
    return x, labels, K


def _within(name, key, got, ref, dev_name, floor, who, achieved):
    """got against ref within MARGIN x dev_<dev_name>: NaN where ref is NaN, 0 where ref is 0, else relative to max(|ref|, floor)"""
    got, ref = np.atleast_1d(np.asarray(got, np.float64)), np.atleast_1d(np.asarray(ref, np.float64))
    assert got.shape == ref.shape, (who, name, key)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), (who, name, key, "NaN placement")
    ok = np.isfinite(ref)
    zero = ok & (ref == 0) & (floor == 0)
    assert np.all(got[zero] == 0), (who, name, key, "an exact 0 is not met")
    rest = ok & ~zero
    if not rest.any():
        return
    e = float(np.max(np.abs(got[rest] - ref[rest]) / np.maximum(np.abs(ref[rest]), floor)))
    bound = MARGIN * float(golden()["dev_" + dev_name])
    achieved[dev_name] = max(achieved.get(dev_name, 0.0), e)
    print("%s %s %s: deviation %.3e, bound %.3e (16 x dev_%s)" % (who, name, key, e, bound, dev_name))
    assert e <= bound, (who, name, key, e, bound)


def check_against_golden(name, got, who):
    """got: a dict with any of the parameter and result arrays of fixture `name` -> the achieved deviation per dev_<q>"""
    g = golden()
    achieved = {}
    for key in EQUAL:
        if key in got:
            assert np.array_equal(np.asarray(got[key]), g["%s/%s" % (name, key)]), (who, name, key)
    for key, (dev_name, floor) in FLOATS.items():
        if key in got:
            _within(name, key, got[key], g["%s/%s" % (name, key)], dev_name, floor, who, achieved)
    use = g[name + "/use_g"]
    big = g[name + "/below_median"] != 255
    exact = ~big & use[None, :]
    if "p_values" in got:
        p = np.asarray(got["p_values"])
        assert np.all(p[:, ~use] == 1.0), (who, name, "p of a gene that is not used")
        if exact.any():
            _within(name, "p_values (exact)", p[exact], g[name + "/mp_p"][exact], "exact_p", 0.0, who, achieved)
        if big.any():
            _within(name, "p_values (asymptotic)", p[big], g[name + "/mp_p"][big], "asymptotic_p", 0.0, who, achieved)
    if "adjusted_p_values" in got:
        q = np.asarray(got["adjusted_p_values"])
        assert np.all(q[:, ~use] == 1.0), (who, name, "adjusted p of a gene that is not used")
        _within(name, "adjusted_p_values", q[:, use], g[name + "/mp_adj"][:, use], "adjusted_p", 0.0, who, achieved)
    return achieved


def test_hand_case_poisson():
    x = np.array([[1, 1, 1, 1], [2, 0, 2, 0], [1, 3, 1, 3]])
    P = R.compute_params(x)
    assert P["size_factors"].tolist() == [1.0] * 4 and P["mean_g"].tolist() == [1.0, 1.0, 2.0] and P["var_g"].tolist() == [0.0, 1.0, 1.0]
    assert P["use_g"].tolist() == [False, True, True] and P["phi_mm_g"].tolist() == [0.0, 0.0, 0.0] and P["zeta_hat"] == 0.0 and np.isnan(P["delta"])
    assert np.isnan(P["phi_g"][0]) and P["phi_g"][1:].tolist() == [0.0, 0.0]
    o = R.diffexp(x, P, [1, 2, 1, 2], 2)
    assert o["sums_in"].tolist() == [[2, 4, 2], [2, 0, 6]] and o["sums_out"].tolist() == [[2, 0, 6], [2, 4, 2]] and o["s_a"].tolist() == [2.0, 2.0]
    for c in (0, 1):
        assert o["p_values"][c, 0] == 1.0 and o["adjusted_p_values"][c, 0] == 1.0
        assert abs(o["p_values"][c, 1] - 2 / 16) < 1e-15 and abs(o["p_values"][c, 2] - 74 / 256) < 1e-15
        assert abs(o["adjusted_p_values"][c, 1] - 0.25) < 1e-15 and abs(o["adjusted_p_values"][c, 2] - 74 / 256) < 1e-15
    assert np.array_equal(o["p_values"][0], o["p_values"][1])      # the mirrored cluster, bit for bit
    assert o["norm_mean_in"][0].tolist() == [1.0, 2.0, 1.0] and abs(o["log2_fold_change"][0, 1] - np.log2(5.0)) < 1e-15
    assert o["n_exact"].tolist() == [2, 2] and o["n_asymptotic"].tolist() == [0, 0] and o["data"].shape == (3, 6)
    assert np.array_equal(o["data"][:, 3], o["norm_mean_in"][1]) and np.array_equal(o["data"][:, 5], o["adjusted_p_values"][1])


def test_hand_case_shrinkage():
    P = R.compute_params(np.array([[1, 1, 1, 1], [4, 0, 0, 0], [0, 4, 4, 4]]))
    delta = 1 / 3.9602
    assert P["use_g"].tolist() == [False, True, True] and P["phi_mm_g"].tolist() == [0.0, 2.0, 0.0] and P["n_used"] == 2
    assert abs(P["zeta_hat"] - 1.99) < 1e-15 and abs(P["delta"] - delta) < 1e-13
    assert np.isnan(P["phi_g"][0]) and abs(P["phi_g"][1] - (2 - 0.01 * delta)) < 1e-13 and abs(P["phi_g"][2] - 1.99 * delta) < 1e-13


def test_refusals_of_the_restatement():
    ok = np.array([[1, 1, 1, 1], [4, 0, 0, 0], [0, 4, 4, 4]])
    for bad in (ok[:2], ok[:, :1], np.array([[1, 0], [1, 0], [2, 0]]), np.ones((3, 4), int)):
        with pytest.raises(ValueError):
            R.compute_params(bad)
    P = R.compute_params(ok)
    for labels, K in (([1, 1, 1, 1], 1), ([1, 2, 3, 1], 2), ([0, 1, 2, 1], 2), ([1, 1, 1, 1], 2), ([1, 2, 1], 2)):
        with pytest.raises(ValueError):
            R.diffexp(ok, P, labels, K)


def test_bh_with_ties():
    q = R.adjust_bh([0.01, 0.04, 0.04, 0.03, 0.5])
    assert np.allclose(q, [0.05, 0.05, 0.05, 0.05, 0.5], rtol=0, atol=1e-16) and q[1] == q[2]
    assert R.adjust_bh([0.3]).tolist() == [0.3] and R.adjust_bh([0.9, 0.8]).tolist() == [0.9, 0.9] and len(R.adjust_bh([])) == 0


def test_two_tiny_tests_against_exact_arithmetic():
    for xa, xb, sa, sb, mu, phi in ((3, 7, 1.3, 2.1, 1.7, 0.4), (5, 1, 0.8, 3.3, 0.6, 0.0)):
        assert abs(R.exact_p(xa, xb, sa, sb, mu, phi) / float(R.exact_p_mp(xa, xb, sa, sb, mu, phi)) - 1) < 1e-13
    p, left, _ = R.asymptotic_p(950, 1200, 10.0, 12.0, 95.0, 0.3)
    q, left_mp, _ = R.asymptotic_p_mp(950, 1200, 10.0, 12.0, 95.0, 0.3)
    assert left == left_mp and abs(p / float(q) - 1) < 1e-12


@pytest.mark.parametrize("name", sorted(R.FIXTURES))
def test_restatement_equals_the_golden_file(name):
    x, labels, K = fixture(name)
    P = R.compute_params(x)
    got = dict(P)
    got.update(R.diffexp(x, P, labels, K))
    check_against_golden(name, got, "restatement")
    assert np.array_equal(np.isnan(P["phi_g"]), ~P["use_g"])


def test_what_the_fixtures_cover():
    g = golden()
    assert int(g["n_rejected"]) * 8 <= len(R.FIXTURES)
    assert g["two_cells_one_cluster/labels"].tolist() == [1, 2]
    assert not g["constant_rows/use_g"][:3].any() and g["constant_rows/use_g"][3:].all()
    assert np.all(g["poisson/phi_mm_g"] == 0) and np.isnan(float(g["poisson/delta"])) and np.all(g["poisson/phi_g"] == 0)
    assert g["mirror/s_a"][0] == g["mirror/s_b"][0] and np.array_equal(g["mirror/p_values"][0], g["mirror/p_values"][1])
    lt_in, lt_out = g["long_tail/sums_in"][0], g["long_tail/sums_out"][0]
    assert lt_in[0] <= 5 and lt_out[0] == 70000 and lt_in[1:4].tolist() == [899, 900, 901] and lt_out[4:7].tolist() == [899, 900, 901]
    assert (g["long_tail/below_median"][0, 1:7] != 255).tolist() == [False, False, True, False, False, True]      # > 900 on both sides
    assert g["k10/sums_in"].shape == (10, 30) and g["g3/sums_in"].shape == (2, 3) and g["base/n_asymptotic"].sum() > 0
