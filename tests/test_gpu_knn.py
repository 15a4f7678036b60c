"""GPU tests of the k-nearest-neighbour stage (Context.knn, engine.run_graph_clustering; csrc/knn.hip).

Every fixture of tests/knn_numpy.py goes through Context.knn.  Equal with NO tolerance: indices, distances and sorted_indices against
scikit-learn 1.7.2's BallTree as recorded in tests/golden/knn_reference.npz (a seeded sample of the rows; tests/test_knn_restatement.py
says how) and, over every row, against the restatement, which the CPU tests pin to BallTree; mid_5000 against the restatement alone.  On
the tied fixtures the distances equal BallTree's and the indices are the (d2, index) order.  Bit for bit: run against run, the smallest
buffer the capacity seam allows (with more than one compaction per query tile on `approach`), the buffers forced into device memory,
candidate tiles of 4 and 12 rows, query ranges against the same rows of the whole, num_pcs as a view against the sliced copy.
engine.run_graph_clustering on rule_2000 and, with a stub for the louvain binary, on the far-apart clusters; the refusals with a live
context, after which the context still works."""
import io

import numpy as np
import pytest

import knn_numpy as R
from test_knn_restatement import GOLDEN

pytestmark = pytest.mark.gpu
EINVAL = -1
_CTX = []
KEYS = ("indices", "distances", "sorted_indices")


def ctx():
    import gpu_helpers as G

    if not _CTX:
        _CTX.append(G.fresh_ctx())
    return _CTX[0]


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def _query(name, **kw):
    f = R.FIXTURES[name]
    return ctx().knn(f["x"], f["k"], num_pcs=f["num_pcs"], **kw)


def _bits(r, lo=None, hi=None):
    return {k: np.ascontiguousarray(r[k][lo:hi]).tobytes() for k in KEYS}


_whole = {}


def whole(name):
    """the default query of a fixture, run once and shared"""
    if name not in _whole:
        _whole[name] = _query(name)
    return _whole[name]


@pytest.mark.parametrize("name", list(R.FIXTURES))
def test_fixture_equals_balltree(golden, name):
    f = R.FIXTURES[name]
    n, k = len(f["x"]), f["k"]
    r = whole(name)
    ind, dist, _ = R.expected(name)
    assert r["indices"].dtype == np.int32 and r["indices"].shape == (n, k) == r["distances"].shape == r["sorted_indices"].shape
    assert np.array_equal(r["indices"], ind)
    assert np.array_equal(r["distances"], dist)                        # every bit, the root included
    assert np.array_equal(r["sorted_indices"], np.sort(ind, axis=1))
    if name not in R.NOT_IN_GOLDEN:
        rows = golden[name + "_rows"]
        assert np.array_equal(r["distances"][rows], golden[name + "_dist"])
        if not f["tied"]:
            assert np.array_equal(r["indices"][rows], golden[name + "_ind"])
            assert np.array_equal(r["sorted_indices"][rows], np.sort(golden[name + "_ind"], axis=1))
        else:
            x = R.used(name)
            for row in rows[:20]:
                assert R.is_pair_order(x, int(row), r["indices"][row], k), row
    # the default buffer: the power of two from 2 (k + 1) up, at least 64; in LDS when 64 of them fit 48 KiB
    cap = max(64, 1 << int(np.ceil(np.log2(2 * (k + 1)))))
    assert r["capacity"] == cap and r["in_lds"] == (cap == 64)
    assert r["pairs_evaluated"] == n * n and r["query_tiles"] == -(-n // R.QUERY_TILE)
    assert n * min(n, k + 1) <= r["survivors"] <= n * n


def test_the_duplicate_quirk_on_the_device():
    r = whole("duplicates")
    for lo, hi in ((7, 150), (40, 41), (3, 299)):
        assert r["indices"][hi, 0] == hi and r["distances"][hi, 0] == 0.0 and lo not in r["indices"][hi]
        assert r["indices"][lo, 0] == hi and r["distances"][lo, 0] == 0.0 and lo not in r["indices"][lo]


@pytest.mark.parametrize("name", ["approach", "n257", "n257_k256", "lattice", "duplicates", "d128", "clustered"])
def test_bit_for_bit_between_runs_and_seams(name):
    k = R.FIXTURES[name]["k"]
    first = _bits(whole(name))
    assert _bits(_query(name)) == first
    small = _query(name, capacity=k + 5)                               # the smallest buffer: four candidates between two looks
    assert _bits(small) == first and small["capacity"] == k + 5
    if name == "n257_k256":
        assert small["compactions"] == 0                               # 257 candidates never fill a buffer of 261
    else:
        assert small["compactions"] > small["query_tiles"] and small["selections"] >= small["compactions"]
    if name == "approach":
        assert small["compactions"] > 10 * small["query_tiles"]       # the later rows keep coming nearer: the buffers fill again and again
        assert whole(name)["compactions"] >= whole(name)["query_tiles"]
    for tile in (4, 12):
        got = _query(name, cand_tile=tile)
        assert _bits(got) == first and got["cand_tile"] == tile
    forced = _query(name, force_device=True)
    assert _bits(forced) == first and not forced["in_lds"]


@pytest.mark.parametrize("name", ["d1", "d3", "offset", "lattice"])
def test_device_memory_forced_where_lds_is_the_default(name):
    assert whole(name)["in_lds"]
    forced = _query(name, force_device=True)
    assert not forced["in_lds"] and _bits(forced) == _bits(whole(name))
    small = _query(name, force_device=True, capacity=R.FIXTURES[name]["k"] + 5)
    assert not small["in_lds"] and _bits(small) == _bits(whole(name)) and small["compactions"] > small["query_tiles"]


@pytest.mark.parametrize("name", ["d3", "approach"])
def test_query_ranges_equal_the_rows_of_the_whole(name):
    n = len(R.FIXTURES[name]["x"])
    for q0, nq in ((0, 1), (n - 1, 1), (100, 257)):
        r = _query(name, query_start=q0, n_queries=nq)
        assert r["indices"].shape[0] == nq and r["pairs_evaluated"] == nq * n
        assert _bits(r) == _bits(whole(name), q0, q0 + nq), (q0, nq)


def test_three_ranges_tile_n257():
    for name in ("n257", "n257_k256"):
        parts = [_query(name, query_start=q0, n_queries=nq) for q0, nq in ((0, 64), (64, 100), (164, 93))]
        for key in KEYS:
            assert np.array_equal(np.concatenate([p[key] for p in parts]), whole(name)[key]), (name, key)


def test_num_pcs_is_a_view():
    f = R.FIXTURES["view"]
    copy = ctx().knn(np.ascontiguousarray(f["x"][:, :10]), f["k"])
    assert _bits(copy) == _bits(whole("view"))
    assert _bits(ctx().knn(f["x"], f["k"])) != _bits(copy)            # all 16 columns: another question


def test_run_graph_clustering_on_rule_2000():
    from cellranger_amd import engine as E

    x = R.FIXTURES["rule_2000"]["x"]
    out = E.run_graph_clustering(ctx(), x, queries_per_call=700)      # three calls, as the reference's chunks
    ind, dist, _ = R.expected("rule_2000")
    assert out["num_neighbors"] == 166 and out["nn_nodes"] == 2000 and out["nn_links"] == 332000 == len(out["nn_indices"])
    assert out["nn_density"] == 332000 / float(2000 * 2000)
    assert np.array_equal(out["indices"], ind) and np.array_equal(out["distances"], dist)
    assert np.array_equal(out["nn_indptr"], np.arange(2001) * 166)
    rows = out["nn_indices"].reshape(2000, 166)
    assert (np.diff(rows, axis=1) > 0).all() and np.array_equal(rows, np.sort(ind, axis=1))
    assert "labels" not in out
    one = E.run_graph_clustering(ctx(), x)
    assert np.array_equal(one["nn_indices"], out["nn_indices"]) and np.array_equal(one["distances"], out["distances"])
    buf = io.StringIO()
    assert E.write_louvain_edges(buf, out["nn_indptr"], out["nn_indices"]) == 332000
    text = buf.getvalue()
    assert text.startswith("0\t%d\n" % rows[0, 0]) and text.endswith("1999\t%d\n" % rows[-1, -1]) and text.count("\n") == 332000
    sparse = pytest.importorskip("scipy.sparse")
    nn = sparse.coo_matrix((2000, 2000))                               # merge_nearest_neighbors over the three chunks, then join()'s tocoo
    for q0 in (0, 700, 1400):
        i = np.repeat(np.arange(q0, min(q0 + 700, 2000)), 166)
        nn = nn + sparse.coo_matrix((np.ones(len(i)), (i, ind[q0:q0 + 700].ravel().astype(int))), shape=nn.shape)
    nn = nn.tocoo()
    assert nn.nnz == 332000 and (nn.data == 1).all()
    assert text == "".join("%d\t%d\n" % ij for ij in zip(nn.row, nn.col))


def _components(row, col, n):
    """stub for the louvain binary: the connected components of the edge list, level 0 as (node, component in order of first
    appearance), then a second level that lists the components again -- which load_louvain_results must skip"""
    lab = np.arange(n)
    while True:
        nxt = lab.copy()
        np.minimum.at(nxt, row, lab[col])
        np.minimum.at(nxt, col, lab[row])
        if np.array_equal(nxt, lab):
            break
        lab = nxt
    _, first, comp = np.unique(lab, return_index=True, return_inverse=True)
    order = np.argsort(np.argsort(first))
    comp = order[comp]
    return [(i, int(c)) for i, c in enumerate(comp)] + [(c, 0) for c in range(int(comp.max()) + 1)]


def test_run_graph_clustering_with_a_louvain_stub():
    from cellranger_amd import engine as E

    x = R.FIXTURES["clustered"]["x"]
    seen = {}

    def louvain(row, col):
        seen["edges"] = len(row)
        return _components(row, col, len(x))

    out = E.run_graph_clustering(ctx(), x, louvain=louvain)
    assert out["num_neighbors"] == 187 and seen["edges"] == 3000 * 187
    # five far clusters of 1000, 800, 600, 400 and 200 rows: 1-based, the largest first
    assert np.array_equal(out["clusters"], R.CLUSTERED_MEMBER + 1)
    assert out["labels"].min() == 1 and len(np.unique(out["labels"])) == 5
    assert np.array_equal(out["clusters"], E.relabel_by_size(out["labels"]))
    # a subsample of the barcodes: 3000 rows out of 3100, the rest get 0 and rank with the clusters as in the reference
    use_bcs = np.arange(3100)[::-1][:3000]
    sub = E.run_graph_clustering(ctx(), x, louvain=louvain, num_barcodes=3100, use_bcs=use_bcs)
    assert (sub["labels"][:100] == 0).all() and np.array_equal(sub["labels"][use_bcs], out["labels"])


def test_refusals_with_a_live_context():
    from cellranger_amd import _lib

    c = ctx()
    x = np.array(R.FIXTURES["d3"]["x"])
    for bad in (np.nan, np.inf, -np.inf):
        y = x.copy()
        y[699, 2] = bad
        with pytest.raises(_lib.CrgpuError) as e:
            c.knn(y, 20)
        assert e.value.code == EINVAL and "not finite" in str(e.value)
    big = np.zeros((1100, 2))
    big[:, 0] = np.arange(1100)
    wide = np.zeros((10, 129))
    for args, kw in (((x, 700), {}), ((big, 1025), {}), ((wide, 3), {}), ((x, 20), dict(num_pcs=4)), ((x, 20), dict(num_pcs=0)),
                     ((x[:1], 1), {}), ((x, 20), dict(capacity=24)), ((x, 20), dict(capacity=4097)), ((x, 20), dict(cand_tile=6)),
                     ((x, 20), dict(cand_tile=260))):
        with pytest.raises((_lib.CrgpuError, ValueError)) as e:
            c.knn(*args, **kw)
        assert not isinstance(e.value, _lib.CrgpuError) or e.value.code == EINVAL, (args[1], kw)
    for q0, nq in ((700, 1), (600, 101), (0, 0)):
        with pytest.raises((_lib.CrgpuError, ValueError)):
            c.knn(x, 20, query_start=q0, n_queries=nq)
    r = c.knn(big, 1024)                                               # the limit itself: points on a line
    assert np.array_equal(r["sorted_indices"][0], np.arange(1, 1025)) and np.array_equal(r["distances"][0], np.arange(1.0, 1025.0))
    assert _bits(c.knn(x, 20)) == _bits(whole("d3"))                  # the context still works
