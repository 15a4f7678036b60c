"""GPU tests of the k-means stage (Context.kmeans, engine.run_kmeans; csrc/kmeans.h).

Every fixture of tests/golden/kmeans_reference.npz goes through Context.kmeans, all the K of a fixture in ONE call.  The expected values
are scikit-learn 1.7.2's, recorded by scripts/make_kmeans_golden.py (tests/test_kmeans_restatement.py says how, and holds the check
shared with the restatement).  Equal with no tolerance: labels, relabelled clusters, n_iter, the strict flag, the relocation count,
sizes.  Within 16 x the largest movement of the quantity between three orders of the sums over cells, read from the file and nowhere
else: centres (absolute against the data's largest magnitude), inertia, wss and the Davies-Bouldin score (relative).  Bit for bit:
run against run, CRGPU_KM_LDS_CENTERS = 0, CRGPU_KM_BATCH = 1 and 7, K = 5 alone against K = 5 inside the list 2 .. 10, num_pcs as a
view against the sliced copy."""
import numpy as np
import pytest

import kmeans_numpy as R
from test_kmeans_restatement import check_against_golden, fixture, golden

pytestmark = pytest.mark.gpu
EINVAL = -1
_CTX = []
FLOATS = ("centers", "inertia", "wss", "db_score")
KEYS = ("labels", "clusters", "centers", "inertia", "wss", "db_score", "sizes", "n_iter", "strict", "relocations")


def ctx():
    import gpu_helpers as G

    if not _CTX:
        _CTX.append(G.fresh_ctx())
    return _CTX[0]


def _fit(c, name, ks=None):
    X, init, max_iter = fixture(name)
    ks = R.FIXTURES[name]["ks"] if ks is None else ks
    return c.kmeans(X, ks, seed=0, init=None if init is None else [init] * len(ks), max_iter=max_iter)


def _bits(fits):
    return [{k: np.asarray(f[k]).tobytes() for k in KEYS} for f in fits]


@pytest.mark.parametrize("name", sorted(R.FIXTURES))
def test_fixture_equals_scikit_learn(name):
    fits = _fit(ctx(), name)
    assert [f["n_clusters"] for f in fits] == R.FIXTURES[name]["ks"]
    for f in fits:
        check_against_golden(name, f["n_clusters"], f, "device")
        d = R.FIXTURES[name]["d"]
        assert f["in_lds"] == (f["n_clusters"] * d <= 4096)
        assert f["db_score"] == R.db_index(f["centers"], f["wss"], f["sizes"])
    if name == "k64_d128":
        assert not fits[0]["in_lds"]      # the one fixture whose centres stay in device memory by default


@pytest.mark.parametrize("name", ["list_2_10", "n257", "far_init", "three_points"])
def test_bit_for_bit_between_runs_and_switches(name, monkeypatch):
    import gpu_helpers as G

    monkeypatch.delenv("CRGPU_KM_BATCH", raising=False)
    monkeypatch.delenv("CRGPU_KM_LDS_CENTERS", raising=False)
    first = _bits(_fit(ctx(), name))
    assert _bits(_fit(ctx(), name)) == first
    for var, value in (("CRGPU_KM_LDS_CENTERS", "0"), ("CRGPU_KM_BATCH", "1"), ("CRGPU_KM_BATCH", "7")):      # read when the context is created
        monkeypatch.setenv(var, value)
        c = G.fresh_ctx()
        got = _fit(c, name)
        assert _bits(got) == first, (var, value)
        if var == "CRGPU_KM_LDS_CENTERS":
            assert not any(f["in_lds"] for f in got)
        c.close()
        monkeypatch.delenv(var)


def test_alone_or_in_a_list():
    both = _fit(ctx(), "list_2_10")
    for k in (5, 10):
        alone = _fit(ctx(), "list_2_10", [k])
        assert _bits(alone) == _bits([f for f in both if f["n_clusters"] == k])
    assert _bits(_fit(ctx(), "list_2_10", [10, 2, 5])) == _bits([f for k in (10, 2, 5) for f in both if f["n_clusters"] == k])


def test_num_pcs_is_a_view():
    X, _, _ = fixture("list_2_10")
    view = ctx().kmeans(X, [2, 5], num_pcs=4)
    copy = ctx().kmeans(np.ascontiguousarray(X[:, :4]), [2, 5])
    assert _bits(view) == _bits(copy) and view[0]["centers"].shape == (2, 4)
    ref = R.fit(X[:, :4], 5)
    assert np.array_equal(view[1]["labels"], ref["labels"]) and view[1]["n_iter"] == ref["n_iter"]


def test_run_kmeans_keys_and_the_cap_by_the_cell_count():
    from cellranger_amd import engine as E

    X, _, _ = fixture("list_2_10")
    out = E.run_kmeans(ctx(), X)
    assert list(out) == ["kmeans_%d_clusters" % k for k in range(2, 11)]
    g = golden()
    for k in range(2, 11):
        r = out["kmeans_%d_clusters" % k]
        assert np.array_equal(r["clusters"], g["list_2_10/k%d/clusters" % k]) and r["num_clusters"] == k and r["centers"].shape == (k, 10)
        assert abs(r["cluster_score"] - float(g["list_2_10/k%d/db_score" % k])) <= 16.0 * float(g["move_score"]) * float(g["list_2_10/k%d/db_score" % k])
    small = E.run_kmeans(ctx(), X[:4], library_prefix="gene_expression")      # four cells: K = 2, 3, 4 only
    assert list(small) == ["gene_expression_kmeans_%d_clusters" % k for k in (2, 3, 4)]
    assert sorted(small["gene_expression_kmeans_4_clusters"]["clusters"].tolist()) == [1, 2, 3, 4]
    assert E.run_kmeans(ctx(), X[:1]) == {}


def test_refusals_with_a_live_context():
    from cellranger_amd import _lib

    X = np.zeros((4, 3))
    for ks, kw in (([0], {}), ([65], {}), ([5], {}), ([2, 2], {}), ([2], dict(num_pcs=4)), ([2], dict(max_iter=0))):
        with pytest.raises(_lib.CrgpuError) as e:
            ctx().kmeans(X, ks, **kw)
        assert e.value.code == EINVAL, (ks, kw)
    with pytest.raises(_lib.CrgpuError) as e:
        ctx().kmeans(np.zeros((4, 129)), [2])
    assert e.value.code == EINVAL
    bad = np.zeros((4, 3))
    bad[2, 1] = np.nan
    with pytest.raises(_lib.CrgpuError):
        ctx().kmeans(bad, [2])
    ok = ctx().kmeans(np.arange(12.0).reshape(4, 3), [1, 4])      # the context is still good
    assert ok[0]["sizes"].tolist() == [4] and sorted(ok[1]["sizes"].tolist()) == [1, 1, 1, 1] and ok[1]["inertia"] == 0.0
