"""GPU tests of RUN_TSNE through the ABI (Context.tsne_affinities, Context.tsne_gradient, Context.tsne, engine.run_tsne; csrc/tsne.hip)
against tests/golden/tsne_reference.npz and the restatement tests/tsne_numpy.py, which the CPU tests pin to scikit-learn 1.7.2 and mpmath.

Affinities: beta, the step counts, indptr and indices equal the file (the maker rejected every fixture with a search step within 1e-9
of a decision, so a last bit of exp cannot turn one); the values lie within a bound derived beside the check from a 1-ulp exp on both
sides.  Gradient: bit-equal to the restatement (the descent holds + - * / only) and within the file's bound of scikit-learn's gradient
/ 4; at constructed sizes around the row tile and CRGPU_TSNE_CAND_CHUNK, with a hub row, coincident rows, twelve decades and every seam
at two settings, bit for bit.  Trajectory: from the device's own P the restatement's Y, uY and gains are bit-equal after 1, 99, 100,
101, 120, 121 and 300 iterations; one call equals two; two runs are identical.  End to end: engine.run_tsne on the three groups, then
Context.kmeans at K = 3; the cost within the file's margin; the all-zero case; theta ignored.  Refusals with a live context."""
import numpy as np
import pytest

import tsne_numpy as R
from test_tsne_restatement import GOLDEN

pytestmark = pytest.mark.gpu
EINVAL = -1
_CTX = []


def ctx():
    import gpu_helpers as G

    if not _CTX:
        _CTX.append(G.fresh_ctx())
    return _CTX[0]


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


_aff = {}


def device_affinities(name):
    """Context.tsne_affinities of a fixture, run once and shared; treat as read-only"""
    if name not in _aff:
        a = R.prepared(name)
        _aff[name] = ctx().tsne_affinities(a["nn_indices"], a["nn_distances"], a["perplexity"])
    return _aff[name]


def _value_bound(a):
    """|device - restatement| of a value of P, relative.  A conditional p_m = exp(-bd_m) / s: bd_m is exact on both sides (one product
    of the same operands); exp within 1 ulp = 2^-52 of exact on each side (OCML there, libm here): 2 * 2^-52 between them; s adds k
    such terms, each off by at most that, plus k roundings on each side; the division one rounding on each side: (4 + 2 k + 2) 2^-53
    + 4 2^-53.  (p_ij + p_ji) / 2: positive terms keep the relative error, one rounding more on each side.  The total: positive terms,
    at most 256 + partials additions on each side; the final division one rounding on each side."""
    k = a["k"]
    cond = (4 + 2 * k + 2 + 4) * 2.0 ** -53
    parts = -(-len(a["values"]) // R.PART_ROWS)
    return 2 * cond + (2 + 2 * (R.PART_ROWS + parts) + 2) * 2.0 ** -53


@pytest.mark.parametrize("name", list(R.FIXTURES) + list(R.NOT_IN_GOLDEN))
def test_affinities(golden, name):
    a, r = R.prepared(name), device_affinities(name)
    expect = {k: golden["%s_%s" % (name, k)] for k in ("beta", "steps", "indptr", "indices", "values")} if name in R.FIXTURES else a
    assert np.array_equal(r["beta"], expect["beta"]) and np.array_equal(r["steps"], expect["steps"])
    assert np.array_equal(r["indptr"], expect["indptr"]) and np.array_equal(r["indices"], expect["indices"])
    assert r["nnz"] == len(expect["values"]) and r["max_steps"] == expect["steps"].max()
    bound = _value_bound(a)
    v, w = r["values"], expect["values"]
    # an exp below the normal range (bd > 693) is a denormal on both sides, each within one spacing 2^-1074 of exact: 2 * 2^-1074 / s
    # of the conditional p, absolutely; through the merge and the division that is the same sum the values themselves take
    cond_allow = bound * a["cond"] + 2 * 2.0 ** -1074 / a["s"][:, None]
    allow = R.symmetrize(a["nn_indices"], cond_allow)[2] / a["p_total"] + bound * w
    worst = float((np.abs(v - w) / allow).max())
    print("%s: the worst |value - restatement| is %.3f of its allowance (relative part %.3g); conditional rows %.3f" % (
        name, worst, bound, float((np.abs(r["cond"] - a["cond"]) / np.maximum(cond_allow, 1e-300)).max())))
    assert worst <= 1.0 and (np.abs(r["cond"] - a["cond"]) <= cond_allow).all()
    assert abs(r["p_total"] - a["p_total"]) <= bound * a["p_total"]
    again = ctx().tsne_affinities(a["nn_indices"], a["nn_distances"], a["perplexity"])
    assert all(np.asarray(again[k]).tobytes() == np.asarray(r[k]).tobytes() for k in ("beta", "steps", "cond", "indptr", "indices", "values"))


@pytest.mark.parametrize("name", R.SKLEARN_FIXTURES)
def test_gradient_on_the_files_p(golden, name):
    csr = tuple(golden["%s_%s" % (name, k)] for k in ("indptr", "indices", "values"))
    for Y, g, kl, gb, kb in zip(golden[name + "_Y"], golden[name + "_grad"], golden[name + "_kl"], golden[name + "_grad_bound"], golden[name + "_kl_bound"]):
        r = ctx().tsne_gradient(*csr, Y)
        dC, Z = R.gradient(*csr, Y)
        assert np.array_equal(r["grad"], dC) and r["sum_q"] == Z      # + - * / only: every bit
        assert np.abs(r["grad"] - g).max() <= gb
        # the cost holds a log: OCML's within 1 ulp = 2^-52 of exact, libm's too, of a quotient that is the same on both sides; a
        # term p log(.) differs by 2 * 2^-52 of itself plus one rounding of the product on each side: 6 * 2^-53 |term|; the sums
        # add, on each side, at most (longest row + 256 + partials) roundings of the sum of |terms|
        q = R._entry_terms(csr[0], csr[1], Y)[1]
        terms = np.abs(csr[2] * np.log((csr[2] + R.FLT_MIN) / (q / Z + R.FLT_MIN))).sum()
        bound = (6 + 2 * (np.diff(csr[0]).max() + R.PART_ROWS + len(Y) / R.PART_ROWS + 1)) * 2.0 ** -53 * terms
        print("%s: |kl - restatement| = %.3g of %.3g, |kl - sklearn| = %.3g" % (name, abs(r["kl"] - R.cost(*csr, Y, Z)), bound, abs(r["kl"] - kl)))
        assert abs(r["kl"] - R.cost(*csr, Y, Z)) <= bound and abs(r["kl"] - kl) <= kb + bound


SHAPES = [(63, 2, 0.0), (64, 3, 0.0), (65, 2, 12.0), (129, 3, 0.0), (R.CAND_CHUNK - 1, 3, 0.0), (R.CAND_CHUNK, 2, 12.0), (R.CAND_CHUNK + 1, 2, 0.0),
          (2 * R.CAND_CHUNK + 1, 2, 0.0)]


@pytest.mark.parametrize("n,dims,decades", SHAPES)
def test_gradient_at_constructed_sizes(n, dims, decades):
    """around the row tile and the candidate chunk; a hub row of n - 1 entries beside rows of 4 and 5, which straddle a wave threshold
    of 5 (and all sit on one side of 4); rows 3 and 4 coincide; |Y| over twelve decades; every seam at two settings"""
    indptr, indices, values, Y = R.synthetic_problem(n, dims, 1000 + n, decades)
    assert np.diff(indptr)[0] == n - 1 and {4, 5} <= set(np.diff(indptr).tolist())
    r = ctx().tsne_gradient(indptr, indices, values, Y, exaggeration=12.0)
    dC, Z = R.gradient(indptr, indices, values, Y, 12.0)
    assert r["n_chunks"] == -(-n // R.CAND_CHUNK) and r["pairs_evaluated"] == n * (n - 1)
    assert r["sum_q"] == Z and np.array_equal(r["grad"], dC)
    for seams in (dict(row_tile=128, cand_tile=1), dict(row_tile=256, cand_tile=1024, slab_rows=256), dict(cand_tile=7, slab_rows=64, wave_row_len=5),
                  dict(wave_row_len=4), dict(wave_row_len=1), dict(wave_row_len=1 << 30, cand_tile=333)):
        if n > R.CAND_CHUNK and seams.get("cand_tile") == 1:
            seams = dict(seams, cand_tile=3)
        s = ctx().tsne_gradient(indptr, indices, values, Y, exaggeration=12.0, **seams)
        assert s["grad"].tobytes() == r["grad"].tobytes() and s["sum_q"] == r["sum_q"] and s["kl"] == r["kl"], seams
        assert seams.get("slab_rows", 0) == 0 or s["n_groups"] == -(-n // seams["slab_rows"])


def test_trajectory_from_the_devices_own_p():
    T = R.TRAJECTORY
    a, P = R.prepared(T["name"]), device_affinities(T["name"])
    csr = (P["indptr"], P["indices"], P["values"])
    kw = dict(max_iter=T["max_iter"], stop_lying_iter=T["stop_lying_iter"], mom_switch_iter=T["mom_switch_iter"])
    kept = R.run(*csr, a["y0"], 0, T["max_iter"], T["stop_lying_iter"], T["mom_switch_iter"], keep=T["keep"])[3]
    y, uY, gains, at = a["y0"], None, None, 0
    for k in T["keep"]:      # the device goes on from its own state: the calls chain to 300
        r = ctx().tsne(*csr, y, uY, gains, first_iter=at, n_iters=k - at, **kw)
        y, uY, gains, at = r["y"], r["uY"], r["gains"], k
        for name, mine, theirs in zip(("Y", "uY", "gains"), (y, uY, gains), kept[k]):
            assert np.array_equal(mine, theirs), "%s after %d iterations: %d of %d values differ" % (name, k, (mine != theirs).sum(), mine.size)
    assert r["kl"] == pytest.approx(R.cost(*csr, y), rel=1e-12)
    one = ctx().tsne(*csr, a["y0"], **kw)
    first = ctx().tsne(*csr, a["y0"], first_iter=0, n_iters=100, **kw)
    two = ctx().tsne(*csr, first["y"], first["uY"], first["gains"], first_iter=100, n_iters=200, **kw)
    again = ctx().tsne(*csr, a["y0"], **kw)
    for k in ("y", "uY", "gains"):
        assert one[k].tobytes() == two[k].tobytes() == again[k].tobytes() == r[k].tobytes(), k
    assert one["kl"] == two["kl"] == again["kl"] and one["sum_q"] == two["sum_q"]
    dims3 = R.prepared("hub")      # three output dimensions, the hub row walked by a wave
    P3 = device_affinities("hub")
    csr3 = (P3["indptr"], P3["indices"], P3["values"])
    r3 = ctx().tsne(*csr3, dims3["y0"], n_iters=30, max_iter=30, stop_lying_iter=10, mom_switch_iter=12)
    Y3, uY3, g3, _ = R.run(*csr3, dims3["y0"], 0, 30, 10, 12)
    assert np.array_equal(r3["y"], Y3) and np.array_equal(r3["uY"], uY3) and np.array_equal(r3["gains"], g3)


def test_end_to_end_three_groups(golden):
    from cellranger_amd import engine

    f = R.FIXTURES["three_groups"]
    out = engine.run_tsne(ctx(), f.x, seed=f.seed)
    assert out["embedding"].shape == (300, 2) and out["perplexity_used"] == 30 and out["num_neighbors"] == 90
    assert (out["name"], out["key"]) == ("gene_expression_2-d", "2")
    labels = ctx().kmeans(out["embedding"], [3])[0]["labels"]
    assert [len(set(labels[g * 100:(g + 1) * 100].tolist())) for g in range(3)] == [1, 1, 1] and len(set(labels.tolist())) == 3
    final, margin = float(golden["three_groups_final_kl"]), float(golden["three_groups_kl_margin"])
    print("kl on the device %.9f, the restatement's %.9f, margin %.3g" % (out["kl"], final, margin))
    assert abs(out["kl"] - final) <= margin
    zero = engine.run_tsne(ctx(), f.x, seed=f.seed, theta=0.0)      # theta is ignored: the same bits
    assert zero["embedding"].tobytes() == out["embedding"].tobytes() and zero["kl"] == out["kl"]
    z = engine.run_tsne(None, R.ALL_ZERO.x)      # no context: nothing can have been launched
    assert z["embedding"].shape == (3, 2) and not z["embedding"].any() and z["perplexity_used"] == 1


def test_refusals_with_a_live_context():
    from cellranger_amd import _lib

    c = ctx()
    a = R.prepared("chain")
    ind, dist = a["nn_indices"], a["nn_distances"]

    def refused(fn, *args, **kw):
        with pytest.raises((_lib.CrgpuError, ValueError)) as e:
            fn(*args, **kw)
        assert not isinstance(e.value, _lib.CrgpuError) or e.value.code == EINVAL, (args[-1] if args else None, kw)

    twice, outside, negative, nan = ind.copy(), ind.copy(), dist.copy(), dist.copy()
    twice[2, 1], outside[3, 0], negative[1, 1], nan[0, 2] = twice[2, 0], len(ind), -1.0, np.nan
    for args in ((ind, dist, 0.5), (ind, dist, np.nan), (twice, dist, 1.0), (outside, dist, 1.0), (ind, negative, 1.0), (ind, nan, 1.0),
                 (ind[:3], dist[:3], 1.0), (ind[:1, :1], dist[:1, :1], 1.0)):
        refused(c.tsne_affinities, *args)
    P = device_affinities("chain")
    csr, y = (P["indptr"], P["indices"], P["values"]), a["y0"]
    swapped, beyond, inf_y = P["indices"].copy(), P["indices"].copy(), y.copy()
    swapped[[0, 1]], beyond[4], inf_y[2, 0] = swapped[[1, 0]], len(y), np.inf
    for fn in (c.tsne_gradient, c.tsne):
        refused(fn, P["indptr"], swapped, P["values"], y)
        refused(fn, P["indptr"], beyond, P["values"], y)
        refused(fn, *csr, inf_y)
        refused(fn, *csr, np.zeros((len(y), 4)))
        for seams in (dict(row_tile=48), dict(cand_tile=1025), dict(row_tile=128, slab_rows=64)):
            refused(fn, *csr, y, **seams)
    refused(c.tsne, *csr, y, first_iter=5, n_iters=6, max_iter=10)
    refused(c.tsne, *csr, y, eta=-1.0)
    again = c.tsne_affinities(ind, dist, a["perplexity"])      # the context still works
    assert again["values"].tobytes() == P["values"].tobytes()
    assert c.tsne_gradient(*csr, y)["sum_q"] == R.gradient(*csr, y)[1]
