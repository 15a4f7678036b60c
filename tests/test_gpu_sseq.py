"""GPU tests of the sSeq differential expression (Context.sseq_params, Context.sseq_diffexp, engine.run_differential_expression;
csrc/sseq.h).

Every fixture of tests/sseq_numpy.py goes through the device.  Equal with no tolerance: use_g, the size factors, sums_in / sums_out,
the exact / asymptotic split and its counts, the NaN and 1 placement, the side of the median every asymptotic test took.  Floats within
16 x dev_<q>, read from tests/golden/sseq_reference.npz and nowhere else (tests/test_sseq_restatement.py holds the check): p-values and
adjusted p-values against the exact (mpmath) values, the parameters and means against the restatement.  Bit for bit: run against
run; the class thresholds forced through the arguments (every test a wave, every test a workgroup, the defaults); a cluster of a
K-labelling against the same cluster in its two-label relabelling; the two clusters of `mirror`.

Achieved on an MI355X (the largest deviation over the fixtures, in front of its bound 16 x dev): see README.md."""
import numpy as np
import pytest

import sseq_numpy as R
from test_sseq_restatement import check_against_golden, fixture, golden

pytestmark = pytest.mark.gpu
EINVAL = -1
WL = 8192
_CTX, _RUNS = [], {}
BITS = ("sums_in", "sums_out", "norm_mean_in", "norm_mean_out", "log2_fold_change", "p_values", "adjusted_p_values", "below_median", "s_a", "s_b",
        "n_exact", "n_asymptotic", "data")
ALL_WAVE, ALL_WG = dict(wave_min=1, wg_min=0xFFFFFFFF), dict(wave_min=1, wg_min=1)


def ctx():
    import gpu_helpers as G

    if not _CTX:
        c = G.fresh_ctx()
        c.set_whitelist(0, np.arange(WL, dtype=np.uint32), length=16)      # rank == value: column k is barcode k
        _CTX.append(c)
    return _CTX[0]


def _matrix(c, x):
    """MatrixDev of the dense features x cells array x"""
    import scipy.sparse as sp

    m = sp.csc_matrix(x)
    m.sort_indices()
    V = x.shape[1]
    seen = np.zeros(c.n_canon, np.uint32)
    seen[:V] = 1
    c.set_counts(0, 0, seen)
    bc = np.repeat(np.arange(V, dtype=np.uint32), np.diff(m.indptr))
    md = c.assemble_matrix_dev(c.upload(bc), c.upload(m.indices.astype(np.uint32)), c.upload(m.data.astype(np.uint32)), len(bc))
    assert md.n_barcodes == V and md.nnz == m.nnz
    return md


def _run(name):
    """the device's parameters and results of a fixture, computed once and left unchanged"""
    if name not in _RUNS:
        x, labels, K = fixture(name)
        m = _matrix(ctx(), x)
        params = ctx().sseq_params(m, n_features=x.shape[0])
        _RUNS[name] = (m, params, params.download(), ctx().sseq_diffexp(m, params, labels, K))
    return _RUNS[name]


def _bits(o, rows=slice(None)):
    """the bytes of every result, of all clusters or of the clusters `rows`"""
    cols = rows if rows.start is None else slice(3 * rows.start, 3 * rows.stop)
    return {k: np.ascontiguousarray(o[k][:, cols] if k == "data" else o[k][rows]).tobytes() for k in BITS}


@pytest.mark.parametrize("name", sorted(R.FIXTURES))
def test_fixture_equals_the_golden_file(name):
    x, labels, K = fixture(name)
    _, _, P, o = _run(name)
    got = dict(P)
    got.update(o)
    achieved = check_against_golden(name, got, "device")
    print("achieved", name, {k: "%.2e" % v for k, v in sorted(achieved.items())})
    assert np.array_equal(np.isnan(P["phi_g"]), ~P["use_g"]) and P["n_used"] == int(P["use_g"].sum())
    assert o["data"].shape == (x.shape[0], 3 * K) and np.array_equal(o["data"][:, 2::3], o["adjusted_p_values"].T)
    assert o["n_short"] + o["n_wave"] + o["n_workgroup"] == int(o["n_exact"].sum())
    assert o["n_terms"] == int((o["sums_in"] + o["sums_out"] + 1)[(o["below_median"] == 255) & P["use_g"][None, :]].sum())
    if name == "long_tail":
        assert o["n_workgroup"] >= 1      # the 70 005-term test takes a workgroup by default
    if name == "two_cells_one_cluster":
        assert o["n_short"] + o["n_wave"] == 24


@pytest.mark.parametrize("name", ["base", "long_tail", "poisson", "k10"])
def test_bit_for_bit_between_runs_and_classes(name):
    x, labels, K = fixture(name)
    m, params, P, first = _run(name)
    again = ctx().sseq_params(m, n_features=x.shape[0])
    P2 = again.download()
    assert all(np.asarray(P[k]).tobytes() == np.asarray(P2[k]).tobytes() for k in P)
    assert _bits(ctx().sseq_diffexp(m, again, labels, K)) == _bits(first)
    for kw in (ALL_WAVE, ALL_WG):
        got = ctx().sseq_diffexp(m, params, labels, K, **kw)
        assert _bits(got) == _bits(first), kw
        assert (got["n_short"], got["n_wave"] if kw is ALL_WG else got["n_workgroup"]) == (0, 0)
    again.free()


@pytest.mark.parametrize("name,cluster", [("base", 2), ("k10", 7)])
def test_a_cluster_alone_or_among_others(name, cluster):
    x, labels, K = fixture(name)
    m, params, _, both = _run(name)
    two = np.where(labels == cluster, 1, 2).astype(np.int32)      # the cluster against the rest
    alone = ctx().sseq_diffexp(m, params, two, 2)
    a, b = _bits(alone, slice(0, 1)), _bits(both, slice(cluster - 1, cluster))
    assert a == b, [k for k in BITS if a[k] != b[k]]


def test_mirror_clusters_are_equal():
    _, _, P, o = _run("mirror")
    assert o["s_a"][0] == o["s_b"][0] == o["s_a"][1]
    assert o["p_values"][0].tobytes() == o["p_values"][1].tobytes() and o["adjusted_p_values"][0].tobytes() == o["adjusted_p_values"][1].tobytes()
    assert np.all(o["p_values"][0][P["use_g"]] < 1.0 + 1e-12) and len(np.unique(o["p_values"][0])) > 5


def test_run_differential_expression():
    from cellranger_amd import engine as E

    x, labels, K = fixture("base")
    m, _, _, first = _run("base")
    m.n_features = x.shape[0]
    two = np.where(labels == 1, 1, 2).astype(np.int32)
    before = getattr(ctx(), "sseq_params_computed", 0)
    out = E.run_differential_expression(ctx(), m, {"kmeans_3_clusters": dict(clusters=labels), "kmeans_2_clusters": two})
    assert ctx().sseq_params_computed == before + 1      # the parameters are computed once
    assert list(out) == ["kmeans_3_clusters", "kmeans_2_clusters"]
    assert out["kmeans_3_clusters"].shape == (x.shape[0], 9) and out["kmeans_3_clusters"].tobytes() == first["data"].tobytes()
    assert out["kmeans_2_clusters"].shape == (x.shape[0], 6) and np.array_equal(out["kmeans_2_clusters"][:, :3], first["data"][:, :3])


def test_refusals_with_a_live_context():
    from cellranger_amd import _lib

    x, labels, K = fixture("g3")
    m, params, _, first = _run("g3")
    for bad, k in ((labels, 1), (np.where(labels == 1, 3, labels), 2), (np.where(labels == 1, 0, labels), 2), (np.ones_like(labels), 2), (labels, 3)):
        with pytest.raises(_lib.CrgpuError) as e:
            ctx().sseq_diffexp(m, params, bad, k)
        assert e.value.code == EINVAL, k
    with pytest.raises(_lib.CrgpuError) as e:
        ctx().sseq_params(m, n_features=2)      # G < 3
    assert e.value.code == EINVAL
    with pytest.raises(_lib.CrgpuError) as e:
        ctx().sseq_params(_run("k10")[0], n_features=R.FIXTURES["k10"]["G"] - 1)      # the matrix holds a row beyond
    assert e.value.code == EINVAL
    other, _, _, _ = _run("two_cells_one_cluster")
    with pytest.raises(_lib.CrgpuError) as e:
        ctx().sseq_diffexp(other, params, np.array([1, 2], np.int32), 2)      # the parameters of a matrix of another shape
    assert e.value.code == EINVAL
    zero = x.copy()
    zero[:, 3] = 0
    with pytest.raises(_lib.CrgpuError) as e:
        ctx().sseq_params(_matrix(ctx(), zero), n_features=3)      # a cell without counts
    assert e.value.code == EINVAL
    assert _bits(ctx().sseq_diffexp(m, params, labels, K)) == _bits(first)      # the context is still good
