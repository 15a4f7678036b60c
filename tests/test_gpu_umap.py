"""GPU tests of RUN_UMAP through the ABI (Context.umap_graph, Context.umap_epochs, engine.run_umap; csrc/umap.hip) against
tests/golden/umap_reference.npz and the restatement tests/umap_numpy.py, which the CPU tests pin to scipy 1.15.3 and mpmath.

Graph: rho, the step counts, indptr and indices equal the file (the maker rejected every fixture with a search step within 1e-9 of a
decision or an entry within 1e-9 of the prune threshold, so a last bit of exp cannot turn one); sigma equals the file because, the
decisions given, the search holds + - * / only; the values lie within a bound derived beside the check from a 1-ulp exp on both sides.
Epochs: one step from the device's own Y and state at the epochs 0, 1, 2, 99, 100 and the last: the active count, the sample count and
both schedule states are bit-equal to the restatement, delta and Y' lie within the per-step bound (pow is OCML's there and libm's
here; the trajectory is not compared across steps, because the descent amplifies a last bit).  One call equals two, two runs are
identical, the seams move no bit, the seed changes the result.  End to end: engine.run_umap on the three groups, then Context.kmeans at
K = 3.  Refusals with a live context."""
import numpy as np
import pytest

import umap_numpy as R
from test_umap_restatement import GOLDEN

pytestmark = pytest.mark.gpu
EINVAL = -1
U = 2.0 ** -53
_CTX = []


def ctx():
    import gpu_helpers as G

    if not _CTX:
        _CTX.append(G.fresh_ctx())
    return _CTX[0]


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


_graph = {}


def device_graph(name):
    """Context.umap_graph of a fixture, run once and shared; treat as read-only"""
    if name not in _graph:
        g = R.prepared(name)
        _graph[name] = ctx().umap_graph(g["nn_indices"], g["nn_distances"], g["n_epochs"])
    return _graph[name]


def _ab():
    from cellranger_amd import engine

    return engine.umap_ab()


def _value_allowance(g):
    """|device - restatement| of a kept value.  A membership exp(-(x / sigma)): x / sigma is the same on both sides (sigma is bit-equal);
    exp within 1 ulp = 2 u of exact on each side (OCML there, libm here; u = 2^-53): 4 u of itself between them, and below the normal
    range each side is within one spacing 2^-1074 of exact.  v = (a + b) - a * b: the sum moves by da + db and is rounded once on each
    side (2 u (a + b)), the product by a db + b da and 2 u a b, the difference is rounded once on each side (2 u v)."""
    a, b, v = g["union_a"][g["keep"]], g["union_b"][g["keep"]], g["values"]
    da, db = 4 * U * a + 2 * 2.0 ** -1074, np.where(b > 0, 4 * U * b + 2 * 2.0 ** -1074, 0.0)
    return (da + db) + (a * db + b * da) + 2 * U * ((a + b) + a * b + v)


@pytest.mark.parametrize("name", list(R.FIXTURES))
def test_graph(golden, name):
    g, r = R.prepared(name), device_graph(name)
    want = {k: golden["%s_%s" % (name, k)] for k in ("rho", "sigma", "steps", "indptr", "indices", "values")}
    assert np.array_equal(r["rho"], want["rho"]) and np.array_equal(r["steps"], want["steps"])
    assert np.array_equal(r["indptr"], want["indptr"]) and np.array_equal(r["indices"], want["indices"])
    assert r["nnz"] == len(want["values"]) and r["max_steps"] == want["steps"].max() and r["wmax"] == 1.0
    assert np.array_equal(r["sigma"], want["sigma"])      # the decisions given, + - * / only
    allow = _value_allowance(g)
    worst = float((np.abs(r["values"] - want["values"]) / allow).max())
    print("%s: the worst |value - file| is %.3f of its allowance" % (name, worst))
    assert worst <= 1.0
    n = len(want["rho"])      # twin entries carry equal bits
    dense = np.zeros((n, n))
    dense[np.repeat(np.arange(n), np.diff(r["indptr"])), r["indices"]] = r["values"]
    assert dense.tobytes() == np.ascontiguousarray(dense.T).tobytes()
    again = ctx().umap_graph(g["nn_indices"], g["nn_distances"], g["n_epochs"])
    assert all(np.asarray(again[k]).tobytes() == np.asarray(r[k]).tobytes() for k in ("rho", "sigma", "steps", "indptr", "indices", "values"))


def _step_allowance(info, Ynew):
    """|device - restatement| of delta and of Y' after one epoch from the same Y and state.  d2 and v are the same on both sides (+ - *
    of the same operands).  p = pow(d2, b) within 1 ulp = 2 u of exact on each side (OCML's documented f64 pow; libm's is within 1 ulp
    too): 4 u between them.  Attraction c = (m2ab * (p / d2)) / (a * p + 1): the quotient 4 u + 2 u, the product 2 u more, the
    denominator 4 u + 2 u (the product) + 2 u (the sum, whose terms are positive), the division 2 u: 18 u; c * v 2 u more: 20 u.  A
    negative sample's c = g2b / ((0.001 + d2) * den): den 8 u, the product 2 u, the division 2 u, c * v 2 u: 14 u.  The clip is
    1-Lipschitz and continuous at +-4, and a clipped term is 4: 20 u |term| holds after it; the factor 2 is exact.  A row's m terms
    are added in one order on both sides: Higham's gamma_m = m u / (1 - m u) of sum |terms| on each side.  Y' = y + alpha * delta: one
    rounding of the product and one of the sum on each side."""
    m = info["n_terms"][:, None].astype(np.float64)
    d_allow = (20 * U + 2 * (m * U / (1 - m * U))) * info["sum_abs"]
    y_allow = info["alpha"] * d_allow + 2 * U * np.abs(info["alpha"] * info["delta"]) + 2 * U * np.abs(Ynew)
    return d_allow, y_allow


def _check_step(csr, Y, eons, eonns, n, n_epochs, a, b, seed, **kw):
    """one epoch on the device and in the restatement from the same Y and state -> (the device's result, the worst ratios)"""
    r = ctx().umap_epochs(*csr, Y, a, b, seed=seed, first_epoch=n, n_run=1, n_epochs=n_epochs, epoch_of_next_sample=eons,
                          epoch_of_next_negative_sample=eonns, want_delta=True, **kw)
    if n == 0:
        eons, eonns = R.schedule(csr[2], float(csr[2].max()), kw.get("negative_sample_rate", R.RATE))
    Ynew, e2, en2, info = R.epoch(*csr, Y, eons, eonns, n, n_epochs, a, b, seed, rate=kw.get("negative_sample_rate", R.RATE), detail=True)
    assert r["n_active"] == info["n_active"] and r["n_negative"] == info["n_negative"], (n, r["n_active"], info["n_active"])
    assert np.array_equal(r["epoch_of_next_sample"], e2) and np.array_equal(r["epoch_of_next_negative_sample"], en2), n
    d_allow, y_allow = _step_allowance(info, Ynew)
    d_diff, y_diff = np.abs(r["delta"] - info["delta"]), np.abs(r["y"] - Ynew)
    assert (d_diff <= d_allow).all() and (y_diff <= y_allow).all(), (n, float((d_diff / np.maximum(d_allow, 1e-300)).max()))
    return r, float((d_diff / np.maximum(d_allow, 1e-300)).max()), float((y_diff / np.maximum(y_allow, 1e-300)).max())


@pytest.mark.parametrize("name", ["three_groups", "hub", "duplicates", "chain"])
def test_one_step_from_the_devices_own_state(name):
    g, G = R.prepared(name), device_graph(name)
    csr = (G["indptr"], G["indices"], G["values"])
    a, b = _ab()
    n_epochs, seed = g["n_epochs"], g["seed"]
    Y, eons, eonns, at, worst = g["y0"], None, None, 0, (0.0, 0.0)
    for n in (0, 1, 2, 99, 100, n_epochs - 1):
        if n > at:      # the device goes on from its own state
            r = ctx().umap_epochs(*csr, Y, a, b, seed=seed, first_epoch=at, n_run=n - at, n_epochs=n_epochs, epoch_of_next_sample=eons,
                                  epoch_of_next_negative_sample=eonns)
            Y, eons, eonns = r["y"], r["epoch_of_next_sample"], r["epoch_of_next_negative_sample"]
        r, wd, wy = _check_step(csr, Y, eons, eonns, n, n_epochs, a, b, seed)
        Y, eons, eonns, at, worst = r["y"], r["epoch_of_next_sample"], r["epoch_of_next_negative_sample"], n + 1, (max(worst[0], wd), max(worst[1], wy))
    print("%s: the worst |delta - restatement| is %.3f of its bound, |Y' - restatement| %.3f" % (name, *worst))
    assert np.isfinite(Y).all()


SHAPES = [(63, 2), (64, 3), (65, 2), (255, 3), (257, 2)]


@pytest.mark.parametrize("n,dims", SHAPES)
def test_seams_cuts_and_seed_at_constructed_sizes(n, dims):
    """around the wave and the row tile; a hub row of n - 1 entries beside rows of 4 and 5, which straddle a wave threshold of 5 (and all
    sit on one side of 4); rows 3 and 4 coincide (d2 = 0); the largest rate (n_neg up to 15); every seam at two settings"""
    indptr, indices, values, Y = R.synthetic_graph(n, dims, 2000 + n)
    assert np.diff(indptr)[0] == n - 1 and {4, 5} <= set(np.diff(indptr).tolist())
    csr = (indptr, indices, values)
    a, b = _ab()
    kw = dict(seed=11, n_epochs=40, negative_sample_rate=8)
    r, wd, wy = _check_step(csr, Y, None, None, 0, 40, a, b, 11, negative_sample_rate=8)
    one = ctx().umap_epochs(*csr, Y, a, b, n_run=12, want_delta=True, **kw)
    first = ctx().umap_epochs(*csr, Y, a, b, n_run=5, **kw)
    two = ctx().umap_epochs(*csr, first["y"], a, b, first_epoch=5, n_run=7, epoch_of_next_sample=first["epoch_of_next_sample"],
                            epoch_of_next_negative_sample=first["epoch_of_next_negative_sample"], want_delta=True, **kw)
    keys = ("y", "epoch_of_next_sample", "epoch_of_next_negative_sample", "delta")
    assert all(one[k].tobytes() == two[k].tobytes() for k in keys)
    assert one["n_active"] == first["n_active"] + two["n_active"] and one["n_negative"] == first["n_negative"] + two["n_negative"]
    _, _, _, totals, _ = R.run(*csr, Y, 0, 12, 40, a, b, 11, rate=8)
    assert (one["n_active"], one["n_negative"]) == (totals["n_active"], totals["n_negative"]) and 8 <= totals["max_n_neg"] <= 15
    for seams in (dict(wave_row_len=5), dict(wave_row_len=4, rows_per_wg=64), dict(wave_row_len=1, rows_per_wg=128), dict(wave_row_len=1 << 30),
                  dict(rows_per_wg=64), dict(wave_row_len=n - 1, rows_per_wg=128), dict(wave_row_len=n)):
        s = ctx().umap_epochs(*csr, Y, a, b, n_run=12, want_delta=True, **kw, **seams)
        assert all(s[k].tobytes() == one[k].tobytes() for k in keys) and (s["n_active"], s["n_negative"]) == (one["n_active"], one["n_negative"]), seams
    other = ctx().umap_epochs(*csr, Y, a, b, n_run=12, **dict(kw, seed=12))
    assert other["y"].tobytes() != one["y"].tobytes() and other["epoch_of_next_sample"].tobytes() == one["epoch_of_next_sample"].tobytes()
    # a twelve-epoch step check further on, where entries of every weight have been active and the self-sample has occurred or not
    _check_step(csr, one["y"], one["epoch_of_next_sample"], one["epoch_of_next_negative_sample"], 12, 40, a, b, 11, negative_sample_rate=8)
    # the smallest rate: the entries of weight 1 are active at epoch 1 with n_neg = 0
    eons, eonns = R.schedule(values, 1.0, 1)
    r1 = _check_step(csr, Y, eons, eonns, 1, 40, a, b, 11, negative_sample_rate=1)[0]
    assert r1["n_active"] == int((values == 1.0).sum()) and r1["n_negative"] == 0


def test_end_to_end_three_groups():
    from cellranger_amd import engine

    f = R.FIXTURES["three_groups"]
    out = engine.run_umap(ctx(), f.x, seed=f.seed)
    assert out["embedding"].shape == (300, 2) and np.isfinite(out["embedding"]).all()
    assert out["num_neighbors"] == 30 and out["n_epochs"] == 500 and (out["name"], out["key"]) == ("gene_expression_2-d", "2")
    assert out["nnz"] == R.prepared("three_groups")["nnz"] and out["max_steps"] == R.prepared("three_groups")["steps"].max()
    labels = ctx().kmeans(out["embedding"], [3])[0]["labels"]
    assert [len(set(labels[g * 100:(g + 1) * 100].tolist())) for g in range(3)] == [1, 1, 1] and len(set(labels.tolist())) == 3
    again = engine.run_umap(ctx(), f.x, seed=f.seed)
    assert again["embedding"].tobytes() == out["embedding"].tobytes()
    other = engine.run_umap(ctx(), f.x, seed=f.seed + 1)
    assert other["embedding"].tobytes() != out["embedding"].tobytes()
    h = R.FIXTURES["hub"]      # three output dimensions, euclidean, a caller's epochs
    three = engine.run_umap(ctx(), h.x, umap_dims=3, n_neighbors=h.n_neighbors, metric="euclidean", seed=h.seed, n_epochs=50)
    assert three["embedding"].shape == (130, 3) and np.isfinite(three["embedding"]).all() and three["name"] == "gene_expression_3-d"
    z = engine.run_umap(None, R.TWO_ROWS.x)      # no context: nothing can have been launched
    assert z["embedding"].shape == (2, 2) and not z["embedding"].any()


def test_refusals_with_a_live_context():
    from cellranger_amd import _lib

    c = ctx()
    g = R.prepared("zero_variance")
    ind, dist = g["nn_indices"], g["nn_distances"]

    def refused(fn, *args, **kw):
        with pytest.raises((_lib.CrgpuError, ValueError)) as e:
            fn(*args, **kw)
        assert not isinstance(e.value, _lib.CrgpuError) or e.value.code == EINVAL, (args[-1] if args else None, kw)

    twice, outside, negative, nan = ind.copy(), ind.copy(), dist.copy(), dist.copy()
    twice[2, 1], outside[3, 0], negative[1, 1], nan[0, 2] = twice[2, 0], len(ind), -1.0, np.nan
    for args in ((ind, dist, 0), (twice, dist, 200), (outside, dist, 200), (ind, negative, 200), (ind, nan, 200), (ind[:3], dist[:3], 200),
                 (ind[:1, :1], dist[:1, :1], 200)):
        refused(c.umap_graph, *args)
    G = device_graph("zero_variance")
    csr, y = (G["indptr"], G["indices"], G["values"]), g["y0"]
    swapped, beyond, inf_y, zero_v = G["indices"].copy(), G["indices"].copy(), y.copy(), G["values"].copy()
    swapped[[0, 1]], beyond[4], inf_y[2, 0], zero_v[5] = swapped[[1, 0]], len(y), np.inf, 0.0
    refused(c.umap_epochs, G["indptr"], swapped, G["values"], y, 1.0, 1.0)
    refused(c.umap_epochs, G["indptr"], beyond, G["values"], y, 1.0, 1.0)
    refused(c.umap_epochs, G["indptr"], G["indices"], zero_v, y, 1.0, 1.0)
    refused(c.umap_epochs, *csr, inf_y, 1.0, 1.0)
    refused(c.umap_epochs, *csr, np.zeros((len(y), 4)), 1.0, 1.0)
    refused(c.umap_epochs, *csr, y, 0.0, 1.0)
    refused(c.umap_epochs, *csr, y, 1.0, float("nan"))
    for kw in (dict(negative_sample_rate=9), dict(rows_per_wg=48), dict(first_epoch=5, n_run=6, n_epochs=10), dict(gamma=-1.0), dict(first_epoch=1),
               dict(first_epoch=1, epoch_of_next_sample=np.full(len(G["values"]), np.nan), epoch_of_next_negative_sample=np.ones(len(G["values"])))):
        refused(c.umap_epochs, *csr, y, 1.0, 1.0, **kw)
    again = c.umap_graph(ind, dist, g["n_epochs"])      # the context still works
    assert again["values"].tobytes() == G["values"].tobytes()
    a, b = _ab()
    _check_step(csr, y, None, None, 0, g["n_epochs"], a, b, g["seed"])
