"""The numpy restatement of RUN_TSNE (tests/tsne_numpy.py) against what does not depend on it (no GPU): scikit-learn 1.7.2's gradient
and cost as recorded in tests/golden/tsne_reference.npz, the conditional rows in mpmath at the restatement's own beta, the maker's
rejection rule, and the constructed properties of the fixtures.  tests/test_gpu_tsne.py then holds the device to the restatement."""
import os

import mpmath
import numpy as np
import pytest

import tsne_numpy as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "tsne_reference.npz")
NEAR = 1e-9      # scripts/make_tsne_golden.py


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.mark.parametrize("name", list(R.FIXTURES))
def test_the_file_is_the_restatement(golden, name):
    a = R.prepared(name)
    for key in ("beta", "steps", "indptr", "indices", "values"):
        assert np.array_equal(golden["%s_%s" % (name, key)], a[key]), key
    # CSR: ascending within a row, symmetric structure, values that add to 1 in the stated order
    n = len(a["x"])
    rows = np.repeat(np.arange(n), np.diff(a["indptr"]))
    keys = rows.astype(np.int64) * n + a["indices"]
    assert (np.diff(keys) > 0).all()
    assert set(keys.tolist()) == set((a["indices"].astype(np.int64) * n + rows).tolist())
    assert abs(R.ordered_sum(a["values"]) - 1.0) < 4 * 2.0 ** -53 * (len(keys) / R.PART_ROWS + R.PART_ROWS)


@pytest.mark.parametrize("name", list(R.FIXTURES) + list(R.NOT_IN_GOLDEN))
def test_no_step_of_a_search_is_near_a_decision(name):
    """the rule the maker rejects by: no |H - log(perplexity)| within 1e-9 of the tolerance or of 0"""
    h = np.abs(R.prepared(name)["hdiff"])
    h = h[np.isfinite(h)]
    bad = int(((np.abs(h - R.TOL) < NEAR) | (h < NEAR)).sum())
    assert bad == 0, "%d of %d steps rejected" % (bad, len(h))


@pytest.mark.parametrize("name", R.SKLEARN_FIXTURES)
def test_gradient_and_cost_agree_with_scikit_learn(golden, name):
    """the restatement's gradient times 4 and its cost against sklearn.manifold._t_sne._kl_divergence at the start, mid-run and the
    end; the bound is the file's: 16 times the restatement's own movement between three candidate orders, floored at one rounding"""
    a = R.prepared(name)
    csr = (a["indptr"], a["indices"], a["values"])
    for Y, g, kl, gb, kb in zip(golden[name + "_Y"], golden[name + "_grad"], golden[name + "_kl"], golden[name + "_grad_bound"], golden[name + "_kl_bound"]):
        dC, Z = R.gradient(*csr, Y)
        dev_g, dev_k = np.abs(dC - g).max(), abs(R.cost(*csr, Y, Z) - kl)
        print("%s: |grad - sklearn / 4| = %.3g of %.3g, |kl - sklearn| = %.3g of %.3g" % (name, dev_g, gb, dev_k, kb))
        assert dev_g <= gb and dev_k <= kb
        # the bounds themselves are a few roundings wide (of the attraction and repulsion that cancel in a late gradient)
        assert gb <= 1e-9 * np.abs(g).max() and kb <= 1e-12 * abs(kl)


def _mp_row(d2, beta):
    bd = [mpmath.mpf(float(beta)) * mpmath.mpf(float(v)) for v in d2]
    p = [mpmath.exp(-v) for v in bd]
    s = mpmath.mpf(R.DBL_MIN) + mpmath.fsum(p)
    H = mpmath.fsum(b * q for b, q in zip(bd, p)) / s + mpmath.log(s)
    return bd, [q / s for q in p], H


@pytest.mark.parametrize("name", list(R.FIXTURES))
def test_rows_in_mpmath_at_their_own_beta(name):
    mpmath.mp.prec = 200
    a = R.prepared(name)
    n, k = a["cond"].shape
    logp = mpmath.log(mpmath.mpf(float(a["perplexity"])))
    rows = np.unique(np.concatenate([np.arange(min(n, 20)), np.arange(n - min(n, 5), n), np.random.RandomState(5).randint(0, n, 15)]))
    worst = 0.0
    for i in rows:
        bd, p, H = _mp_row(a["d2"][i], a["beta"][i])
        if a["steps"][i] < R.MAX_STEPS:
            # converged: the entropy at the reported beta; 1e-5 for the f64 test plus what the f64 H can be off (far below 1e-9)
            assert abs(H - logp) < R.TOL + NEAR, (i, float(H - logp))
            # the bracket: H falls with beta, so a lower bound still has too much entropy and an upper bound too little
            if a["lo"][i] != -R.DBL_MAX:
                assert _mp_row(a["d2"][i], a["lo"][i])[2] > logp
            if a["hi"][i] != R.DBL_MAX:
                assert _mp_row(a["d2"][i], a["hi"][i])[2] < logp
        # p_m = exp(-bd_m) / s.  bd_m is one product: relative 2^-53, which moves exp by bd_m 2^-53; exp within 1 ulp: 2^-52; s is k
        # additions of terms that each carry the largest such error: (max bd + 2) 2^-53 plus k 2^-53; the division 2^-53
        top = max(float(v) for v in bd)
        raw = [mpmath.exp(-v) for v in bd]
        for m in range(k):
            # exp(-bd_m) itself below the normal range (bd_m > 693) is rounded to a denormal, with as few bits as are left: no
            # relative statement there, whatever the size of the quotient; a sum above 2^-960 is untouched by such terms
            if raw[m] < mpmath.mpf(2) ** -1000 or mpmath.fsum(raw) < mpmath.mpf(2) ** -960:
                assert a["cond"][i, m] <= float(p[m]) * 2 + 2.0 ** -50
                continue
            bound = (float(bd[m]) + top + 2 + 2 + k + 1) * 2.0 ** -53
            rel = float(abs(mpmath.mpf(float(a["cond"][i, m])) - p[m]) / p[m])
            worst = max(worst, rel / bound)
            assert rel <= bound, (i, m, rel, bound)
    print("%s: the worst |p - mpmath| is %.3f of its bound" % (name, worst))


def test_the_constructed_properties_of_the_fixtures():
    d = R.prepared("duplicates")
    assert (d["nn_distances"][:17] == 0).all() and (d["steps"][:17] == R.MAX_STEPS).all() and (d["steps"][17:] < R.MAX_STEPS).all()
    assert np.array_equal(d["cond"][:17], np.full((17, d["k"]), 1.0 / (R.DBL_MIN + d["k"])))       # uniform after 200 doublings
    assert (d["nn_indices"][:17] == np.arange(17)[:, None]).any(axis=1).sum() >= 1      # the QUIRK: a row that names itself
    h = R.prepared("hub")
    assert (h["nn_indices"] == 57).any(axis=1).sum() == 129 and np.diff(h["indptr"])[57] == 129      # every row names the hub
    assert np.diff(h["indptr"]).max() == np.diff(h["indptr"])[57] and R.FIXTURES["hub"].dims == 3
    c = R.prepared("chain")
    n, k = c["nn_indices"].shape
    assert k == 3 and c["perplexity"] == 1
    for i in range(n - 4):      # one direction only: i names i + 1 .. i + 3, none of them names i
        assert c["nn_indices"][i].tolist() == [i + 1, i + 2, i + 3] and not (c["nn_indices"][i + 1:i + 4] == i).any()
    assert len(c["values"]) > n * k      # so the union is larger than either direction
    assert R.stage_perplexity(len(R.ALL_ZERO.x), R.ALL_ZERO.perplexity) == (1, True)
    assert R.stage_perplexity(300, 30) == (30, False) and R.stage_perplexity(50, 30)[0] == -1 + 49 / 3.0


def test_the_orders_are_the_stated_ones():
    a = R.prepared("two_groups_130")
    csr = (a["indptr"], a["indices"], a["values"])
    Y = a["y0"] * 1e4
    g0, Z0 = R.gradient(*csr, Y)
    # one chunk: a row's z is its q left to right; written out for three rows
    for i in (0, 64, 129):
        z, neg = 0.0, np.zeros(2)
        for j in range(len(Y)):
            if j == i:
                continue
            v = Y[i] - Y[j]
            q = 1.0 / (1.0 + (v[0] * v[0] + v[1] * v[1]))
            z += q
            neg += (q * q) * v
        zs, negs = R.repulsion(Y)
        assert z == zs[i] and np.array_equal(neg, negs[i])
    # another candidate order moves last bits only, and a trailing zero none
    g1, Z1 = R.gradient(*csr, Y, chunk=7)
    assert np.abs(g1 - g0).max() <= 64 * 2.0 ** -53 * np.abs(g0).max() and abs(Z1 - Z0) <= 64 * 2.0 ** -53 * Z0
    assert R.ordered_sum(np.arange(1000.0)) == R.ordered_sum(np.concatenate([np.arange(1000.0), np.zeros(24)]))
    # sign(0) is 0: a zero velocity and a nonzero gradient differ in sign, the gain grows
    Y1, uY1, gains1 = R.step(*csr, Y, np.zeros_like(Y), np.ones_like(Y), 0, 100, 120)
    assert (gains1[g0 != 0] == 1.2).all() and np.abs(R.ordered_sum(Y1)).max() < 1e-9


def test_the_start_is_the_legacy_generator():
    from cellranger_amd import build, engine

    build.build()
    assert np.array_equal(R.start(7, 130, 3), (engine.legacy_randn(7, 390) * 1e-4).reshape(130, 3))
    x = np.random.RandomState(3).normal(size=(50, 6)) * 7 + 3
    assert np.array_equal(R.normalize(x), engine.tsne_normalize(x))
    assert engine.get_tsne_name("Gene Expression", 2) == "gene_expression_2-d" and engine.get_tsne_key("Gene Expression", 2) == "2"
    assert engine.get_tsne_key("Antibody Capture", 3) == "antibody_capture_3"
