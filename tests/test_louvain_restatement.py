"""The numpy restatement of the Louvain round form (tests/louvain_numpy.py) against hand-computed cases, networkx, scipy and the golden
file (no GPU): the restatement is what the device is compared with bit for bit, so it is pinned here first."""
import os
from fractions import Fraction

import numpy as np
import pytest

import louvain_numpy as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "louvain_reference.npz")
HAND = R.hand_cases()


def _run(name, **kw):
    n, edges, _, _ = HAND[name]
    indptr, indices, w = R.csr_from_edges(n, edges)
    return R.louvain(indptr, indices, w, symmetrize=False, **kw)


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_computed_cases(name):
    _, _, labels, s_m = HAND[name]
    r = _run(name)
    assert r["final"].tolist() == labels
    if s_m:
        assert (r["S"][-1], r["M"]) == s_m
    assert len(set(r["final"].tolist())) == r["communities"][-1]


def test_hand_computed_modularities():
    assert Fraction(70, 14 * 14) == Fraction(5, 14)      # two triangles
    r = _run("path4")
    assert Fraction(r["S"][-1], r["M"] ** 2) == Fraction(1, 6)
    for name in ("one_edge", "star8", "k4"):             # one community: in = tot = M, S = 0
        assert _run(name)["S"][-1] == 0


def test_an_isolated_node_keeps_its_own_community():
    indptr, indices, w = R.csr_from_edges(3, [(0, 1)])
    r = R.louvain(indptr, indices, w, symmetrize=False)
    assert r["final"].tolist() == [0, 0, 1] and r["level0"].tolist() == [0, 0, 1]
    with pytest.raises(ValueError):                      # nothing but isolated nodes: M = 0
        R.louvain(np.zeros(2, np.int64), np.zeros(0, np.int64), None, symmetrize=False)


@pytest.mark.parametrize("name", ["two_triangles", "one_edge", "star8", "path4"])
def test_the_singleton_rule_is_under_test(name):
    """without the rule a plain synchronous round moves nothing useful on these graphs: the result changes"""
    assert _run(name, singleton_rule=False)["final"].tolist() != _run(name)["final"].tolist()


def test_level_zero_without_a_counted_round_is_the_identity():
    indptr, indices, w = R.csr_from_edges(2, [(0, 0), (1, 1)])      # two self-loops: nobody has a neighbour
    r = R.louvain(indptr, indices, w, symmetrize=False)
    assert r["rounds"] == [0] and r["levels"][0].tolist() == [0, 1] and r["final"].tolist() == [0, 1] and r["M"] == 2


def _loop_free_fixtures():
    yield "ring8", 8, R.ring(8)
    yield "ring8_renumbered", 8, R.ring(8, [3, 7, 0, 5, 1, 6, 2, 4])
    for name in ("two_triangles", "star8", "path4", "k4"):
        yield name, HAND[name][0], HAND[name][1]


@pytest.mark.parametrize("name,n,edges", list(_loop_free_fixtures()))
def test_S_is_networkx_modularity_on_loop_free_graphs(name, n, edges):
    nx = pytest.importorskip("networkx")
    G = nx.Graph()
    G.add_nodes_from(range(n))
    G.add_edges_from(edges)
    graph = R.csr_from_edges(n, edges)
    r = R.louvain(*graph, symmetrize=False)
    labellings = r["levels"][:1] + [r["final"], np.arange(n) % 3, np.zeros(n, np.int64)]
    for c in labellings:
        S, M = R.modularity_S(graph, c)
        parts = [set(np.flatnonzero(np.asarray(c) == v).tolist()) for v in np.unique(c)]
        assert abs(S / float(M) ** 2 - nx.community.modularity(G, parts)) < 1e-12


def test_the_union_is_scipys():
    sp = pytest.importorskip("scipy.sparse")
    rs = np.random.RandomState(3)
    n, k = 97, 6
    cols = np.stack([rs.choice(n, k, replace=False) for _ in range(n)])      # a row may name itself: the duplicate quirk
    cols[5, :2] = 5, 5                                                        # and a duplicate within a row
    indptr, indices = np.arange(n + 1, dtype=np.int64) * k, np.sort(cols, axis=1).reshape(-1)
    A = sp.csr_matrix((np.ones(n * k), indices, indptr), shape=(n, n))
    U = ((A + A.T) > 0).tocsr()
    U.sort_indices()
    ptr, ind, w = R.union(indptr, indices)
    assert np.array_equal(ptr, U.indptr) and np.array_equal(ind, U.indices) and (w == 1).all()
    assert (R.csr_rows(ptr) == ind).sum() >= 1
    R.check_symmetric(ptr, ind, w)


def test_aggregation_keeps_M_and_S():
    indptr, indices = R.golden_fixtures()["normal500_k20"]
    graph = R.union(indptr, indices)
    rs = np.random.RandomState(1)
    for groups in (2, 17, 500):
        dense, n_c = R.renumber(rs.randint(0, groups, 500))
        agg = R.aggregate(graph, dense, n_c)
        R.check_symmetric(*agg)
        S, M = R.modularity_S(graph, dense)
        assert R.degrees(agg)[1] == M and R.modularity_S(agg, np.arange(n_c)) == (S, M)
        assert np.array_equal(R.degrees(agg)[0], R.int_bincount(dense, R.degrees(graph)[0], n_c))
        coarse = rs.randint(0, 3, n_c)                  # the induced labelling of a coarser one
        assert R.modularity_S(agg, coarse) == R.modularity_S(graph, coarse[dense])


def test_refusals():
    indptr, indices, w = R.csr_from_edges(4, [(0, 1), (1, 2), (2, 3)])
    for bad in ("order", "twin", "weight", "range", "M"):
        p, i, ww = indptr.copy(), indices.copy(), w.copy()
        if bad == "order":
            i[1], i[2] = i[2], i[1]
        elif bad == "twin":
            ww[0] = 2
        elif bad == "weight":
            ww[0] = ww[1] = 0
        elif bad == "range":
            i[0] = 4
        else:
            ww[:] = 1 << 29
        with pytest.raises(ValueError):
            R.louvain(p, i, ww, symmetrize=False)
    with pytest.raises(ValueError):
        R.louvain(indptr, indices, w, symmetrize=True)


def test_max_rounds_one_ends_every_level_after_a_round():
    indptr, indices = R.golden_fixtures()["groups_s2_k15"]
    r = R.louvain(indptr, indices, max_rounds=1)
    assert set(r["rounds"]) == {1} and len(r["levels"]) > 2
    assert all(a < b for a, b in zip(r["S"], r["S"][1:]))


def test_final_modularity_is_within_the_serial_algorithms_own_spread():
    """Every kNN fixture of the golden file: the round form's final Q is at least networkx's worst Q over 16 seeds minus that fixture's
    spread (maximum minus minimum over the seeds): the margin is the serial algorithm's own sensitivity to its visiting order, taken
    once more.  The three-group fixtures end in the three groups, level 0 refining them into 3 to 7 communities."""
    g = np.load(GOLDEN)
    fixtures = R.golden_fixtures()
    assert sorted(g["names"].tolist()) == sorted(fixtures)
    for name in g["names"].tolist():
        indptr, indices = g[name + "_indptr"], g[name + "_indices"]
        assert np.array_equal(indptr, fixtures[name][0]) and np.array_equal(indices, fixtures[name][1])
        r = R.louvain(indptr, indices)
        M = float(r["M"])
        q0, qf = r["S"][0] / M ** 2, r["S"][-1] / M ** 2
        print("%-18s level 0 %.5f (networkx %.5f .. %.5f), final %.5f (networkx %.5f .. %.5f), rounds %s" % (
            name, q0, g[name + "_q0"].min(), g[name + "_q0"].max(), qf, g[name + "_qfinal"].min(), g[name + "_qfinal"].max(), r["rounds"]))
        assert qf >= g[name + "_qfinal"].min() - g[name + "_spread"][1], name
        assert R.modularity_S(R.union(indptr, indices), r["final"])[0] == r["S"][-1]
        if name.startswith("groups_"):
            assert r["final"].tolist() == np.repeat(np.arange(3), 100).tolist()
            assert 3 <= r["communities"][0] <= 7 and len(set(zip(r["level0"].tolist(), r["final"].tolist()))) == r["communities"][0]
