"""GPU tests of the Louvain stage through the ABI (Context.louvain, engine.run_graph_clustering(louvain="device"); csrc/louvain.hip)
against the restatement tests/louvain_numpy.py, which the CPU tests pin to hand-computed cases, networkx and scipy.

The contract is a synchronous round of exact integers, so nothing here has a tolerance: every level's partition, nodes, communities,
rounds and S, M, level0 and final are equal to the restatement, under every setting of the three seams, in two runs, and with
max_rounds = 1.  Refusals with a live context.  End to end: the three groups through run_graph_clustering into the sSeq stage."""
import numpy as np
import pytest

import louvain_numpy as R

pytestmark = pytest.mark.gpu
EINVAL, ERANGE = -1, -6
WL = 8192
_CTX, _REF = [], {}
SEAMS = (dict(), dict(wave_deg_max=4, lds_deg_max=16, batch=1), dict(wave_deg_max=4), dict(lds_deg_max=16), dict(batch=1))


def ctx():
    import gpu_helpers as G

    if not _CTX:
        c = G.fresh_ctx()
        c.set_whitelist(0, np.arange(WL, dtype=np.uint32), length=16)      # rank == value: column k is barcode k (the end-to-end test)
        _CTX.append(c)
    return _CTX[0]


def _directed(n, edges):
    return R.directed_csr(n, edges) + (None, True)


def _symmetric(n, edges, weights=None):
    return R.csr_from_edges(n, edges, weights) + (False,)


def _fixtures():
    f = {}
    for name, (n, edges, _, _) in R.hand_cases().items():
        f[name] = _symmetric(n, edges)
        f[name + "_directed"] = _directed(n, edges)
    f["isolated"] = _symmetric(3, [(0, 1)])
    f["two_self_loops"] = _symmetric(2, [(0, 0), (1, 1)])      # level 0 without a counted round: the identity
    f["ring8"] = _directed(8, R.ring(8))
    f["ring8_renumbered"] = _directed(8, R.ring(8, [3, 7, 0, 5, 1, 6, 2, 4]))
    f["two_components"] = _directed(9, [(0, 1), (0, 2), (1, 2), (3, 4), (3, 5), (4, 5), (2, 3), (6, 7), (7, 8)])
    for n in (63, 65, 257, 300):
        f["hub%d" % n] = R.hub_rows(n) + (None, True)
    f["weights_2_31"] = _symmetric(4, [(0, 1), (1, 2), (2, 3), (0, 3)], [(1 << 28) - 1, 1 << 28, 1 << 28, 1 << 28])
    rs = np.random.RandomState(4)
    n = 200
    e = np.unique(np.sort(rs.randint(0, n, (900, 2)), axis=1), axis=0)
    f["weighted_random"] = _symmetric(n, e, rs.randint(1, 5000, len(e)))      # self-loops among them: the form of an aggregated level
    return f


FIXTURES = _fixtures()
HUBS = [k for k in FIXTURES if k.startswith("hub")] + ["weighted_random"]


def reference(name):
    """the restatement of a fixture, computed once and shared; treat as read-only"""
    if name not in _REF:
        indptr, indices, w, sym = FIXTURES[name]
        _REF[name] = R.louvain(indptr, indices, w, symmetrize=sym)
    return _REF[name]


def same(dev, ref):
    """every output the contract names, without a tolerance"""
    assert dev["M"] == ref["M"] and dev["nodes"] == ref["nodes"] and dev["communities"] == ref["communities"], (dev["nodes"], ref["nodes"])
    assert dev["rounds"] == ref["rounds"] and dev["S"] == ref["S"], (dev["rounds"], ref["rounds"], dev["S"], ref["S"])
    assert len(dev["levels"]) == len(ref["levels"])
    for a, b in zip(dev["levels"], ref["levels"]):
        assert a.dtype == np.int32 and np.array_equal(a, b)
    assert np.array_equal(dev["level0"], ref["level0"]) and np.array_equal(dev["final"], ref["final"])


def run(name, **kw):
    indptr, indices, w, sym = FIXTURES[name]
    return ctx().louvain(indptr, indices, weights=w, symmetrize=sym, **kw)


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_fixture_equals_the_restatement(name):
    dev, ref = run(name), reference(name)
    same(dev, ref)
    hand = R.hand_cases().get(name.replace("_directed", ""))
    if hand:
        assert dev["final"].tolist() == hand[2] and (hand[3] is None or (dev["S"][-1], dev["M"]) == hand[3])
    assert (dev["wave_deg_max"], dev["lds_deg_max"], dev["batch"]) == (127, 2047, 8)


def test_the_i64_products_at_the_limit():
    dev = run("weights_2_31")
    assert dev["M"] == (1 << 31) - 2 and dev["M"] * (1 << 28) > 1 << 58      # w * M and tot * k beyond 2^58: no i32, no f64 mantissa
    same(dev, reference("weights_2_31"))


@pytest.mark.parametrize("name", HUBS)
@pytest.mark.parametrize("seam", range(1, len(SEAMS)))
def test_no_result_depends_on_a_seam(name, seam):
    """wave_deg_max 4 and lds_deg_max 16 put the hub row (n - 1 entries) on the device-memory table and the rows of 5 to 16 entries on
    a workgroup's LDS table; the defaults put the hub on a workgroup and every other row on a wave; batch 1 reads the latch every round"""
    dev = run(name, **SEAMS[seam])
    same(dev, reference(name))
    want = dict(dict(wave_deg_max=127, lds_deg_max=2047, batch=8), **SEAMS[seam])
    assert {k: dev[k] for k in want} == want


def _knn_graph(seed, k):
    x = R.three_groups(seed)
    r = ctx().knn(x, k)
    return np.arange(len(x) + 1, dtype=np.int64) * k, np.ascontiguousarray(r["sorted_indices"]).reshape(-1)


@pytest.mark.parametrize("k", [15, 67])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_the_three_groups_from_the_device_knn(seed, k):
    """Context.knn's neighbour matrix of three groups of 100 rows: the final partition is the three groups and level 0 refines them
    into 3 to 7 communities; rows of 67 to about 150 entries straddle the default wave and workgroup classes"""
    indptr, indices = _knn_graph(seed, k)
    ref = R.louvain(indptr, indices)
    for kw in (dict(), dict(wave_deg_max=4, lds_deg_max=16, batch=1)):
        same(ctx().louvain(indptr, indices, **kw), ref)
    assert ref["final"].tolist() == np.repeat(np.arange(3), 100).tolist() and 3 <= ref["communities"][0] <= 7
    assert len(set(zip(ref["level0"].tolist(), ref["final"].tolist()))) == ref["communities"][0]      # level 0 refines the groups


def test_coincident_rows_give_self_loops():
    x = np.random.RandomState(11).normal(size=(150, 4))
    for lo, hi in ((7, 90), (40, 41), (149, 3)):      # hi takes lo's row; the one of higher index keeps itself as a neighbour
        x[hi] = x[lo]
    k = 8
    nn = np.ascontiguousarray(ctx().knn(x, k)["sorted_indices"])
    assert (nn == np.arange(150)[:, None]).any(axis=1).sum() == 3
    indptr, indices = np.arange(151, dtype=np.int64) * k, nn.reshape(-1)
    ref = R.louvain(indptr, indices)
    graph = R.union(indptr, indices)
    assert (R.csr_rows(graph[0]) == graph[1]).sum() == 3
    for kw in (dict(), dict(wave_deg_max=4, lds_deg_max=16, batch=1)):
        same(ctx().louvain(indptr, indices, **kw), ref)


def test_two_runs_are_identical():
    for name in ("hub300", "weighted_random"):
        a, b = run(name), run(name)
        same(a, b)
        assert a["nnz"] == b["nnz"]


@pytest.mark.parametrize("name", ["hub257", "weighted_random", "two_triangles"])
def test_max_rounds_one(name):
    indptr, indices, w, sym = FIXTURES[name]
    ref = R.louvain(indptr, indices, w, symmetrize=sym, max_rounds=1)
    assert set(ref["rounds"]) == {1}
    for kw in (dict(), dict(batch=1), dict(wave_deg_max=4, lds_deg_max=16)):
        same(run(name, max_rounds=1, **kw), ref)


def test_refusals_with_a_live_context():
    from cellranger_amd import _lib

    c = ctx()
    indptr, indices, w = R.csr_from_edges(4, [(0, 1), (1, 2), (2, 3)])

    def refused(code, indptr=indptr, indices=indices, weights=w, symmetrize=False, **kw):
        with pytest.raises((_lib.CrgpuError, ValueError)) as e:
            c.louvain(indptr, indices, weights=weights, symmetrize=symmetrize, **kw)
        assert not isinstance(e.value, _lib.CrgpuError) or e.value.code == code, (e.value, kw)
        return e.value

    big, outside, unsorted, unequal, zero, missing = w.copy(), indices.copy(), indices.copy(), w.copy(), w.copy(), indices.copy()
    big[:] = 1 << 29                        # M = 6 * 2^29 >= 2^31
    outside[0] = 4
    unsorted[1], unsorted[2] = indices[2], indices[1]
    unequal[0] = 2                          # (0, 1) weighs 2, (1, 0) weighs 1
    zero[0] = zero[1] = 0                   # both directions: only the weight is wrong
    missing[0] = 2                          # row 0 names 2, row 2 does not name 0
    assert isinstance(refused(ERANGE, weights=big), _lib.CrgpuError)
    for kw in (dict(indices=outside), dict(indices=unsorted), dict(weights=unequal), dict(weights=zero), dict(indices=missing),
               dict(symmetrize=True), dict(wave_deg_max=128), dict(lds_deg_max=2048), dict(indptr=indptr[::-1].copy())):
        assert isinstance(refused(EINVAL, **kw), _lib.CrgpuError), kw
    refused(EINVAL, indptr=np.zeros(2, np.int64), indices=np.zeros(0, np.int32), weights=None)      # no entry: M = 0
    same(run("two_triangles"), reference("two_triangles"))      # the context is still good


def _matrix(c, x):
    """MatrixDev of the dense features x cells array x (as tests/test_gpu_sseq.py builds it)"""
    import scipy.sparse as sp

    m = sp.csc_matrix(x)
    m.sort_indices()
    V = x.shape[1]
    seen = np.zeros(c.n_canon, np.uint32)
    seen[:V] = 1
    c.set_counts(0, 0, seen)
    bc = np.repeat(np.arange(V, dtype=np.uint32), np.diff(m.indptr))
    return c.assemble_matrix_dev(c.upload(bc), c.upload(m.indices.astype(np.uint32)), c.upload(m.data.astype(np.uint32)), len(bc))


def test_run_graph_clustering_on_the_device_end_to_end():
    from cellranger_amd import engine as E

    x = R.three_groups(0)
    out = E.run_graph_clustering(ctx(), x, louvain="device")
    assert out["num_neighbors"] == 67
    ref = R.louvain(out["nn_indptr"], out["nn_indices"])
    same(out["louvain"], ref)
    assert np.array_equal(out["labels"], E.louvain_labels(300, np.arange(300), E.louvain_pairs(out["louvain"])))
    assert np.array_equal(out["labels"], 1 + ref["level0"]) and out["labels"].dtype == np.int64
    assert np.array_equal(out["clusters"], E.relabel_by_size(out["labels"]))
    assert np.array_equal(out["final_clusters"], np.repeat([1, 2, 3], 100))      # equal sizes keep their ascending order
    assert len(out["levels"]) == len(ref["levels"]) and out["modularity"] == [S / float(ref["M"]) ** 2 for S in ref["S"]]
    assert 0.6 < out["modularity"][-1] < 2.0 / 3.0      # three equal groups: Q below 1 - 1/3
    # unused barcodes keep 0 and take part in the ranking, as in the reference
    use = np.arange(300) * 2
    wide = E.run_graph_clustering(ctx(), x, louvain="device", num_barcodes=600, use_bcs=use)
    assert np.array_equal(wide["labels"][use], out["labels"]) and not wide["labels"][use + 1].any()
    assert np.array_equal(wide["labels"], E.louvain_labels(600, use, E.louvain_pairs(wide["louvain"])))
    # the clusters feed the sSeq stage
    rs = np.random.RandomState(0)
    G = 30
    lam = np.full((G, 300), 2.0)
    for g in range(3):
        lam[g * 5:(g + 1) * 5, g * 100:(g + 1) * 100] = 20.0
    counts = rs.poisson(lam)
    counts[0, counts.sum(axis=0) == 0] = 1
    m = _matrix(ctx(), counts)
    m.n_features = G
    de = E.run_differential_expression(ctx(), m, {"graphclust": dict(clusters=out["clusters"].astype(np.int32))})
    K = int(out["clusters"].max())
    assert de["graphclust"].shape == (G, 3 * K) and np.isfinite(de["graphclust"][:, 0]).all()
