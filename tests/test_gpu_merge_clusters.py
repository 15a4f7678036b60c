"""GPU tests of MERGE_CLUSTERS (Context.cluster_medians, engine.merge_clusters, engine.run_graph_clustering(merge_matrix=...);
csrc/merge_clusters.hip, csrc/sseq_pair.h) against tests/golden/merge_clusters_reference.npz, which scripts/make_merge_clusters_golden.py
recorded with scipy's linkage, pandas' groupby median and the stage's own cell order.

Context.cluster_medians equals the file's medoids on every iteration of every fixture (as numbers: an exact selection), and the linkage
of them equals the file's Z bit for bit.  engine.merge_clusters equals the file's step log, counts and labels on every fixture.  On
`oversplit`, run_graph_clustering with a louvain that returns the split labels and merge_matrix gives three merged clusters; without
merge_matrix the dict has the keys it had."""

import numpy as np
import pytest

import merge_clusters_numpy as M
from test_gpu_sseq import _matrix, ctx
from test_merge_clusters_restatement import GOLDEN, check_against_file

pytestmark = pytest.mark.gpu
_REF, _WELLS = [], {}


def ref():
    if not _REF:
        _REF.append(np.load(GOLDEN))
    return _REF[0]


def well(name):
    """the fixture and its device matrix, made once and left unchanged"""
    if name not in _WELLS:
        x, pca, labels = M.fixture(name, int(ref()[name + ".bump"]))
        _WELLS[name] = (x, pca, labels, _matrix(ctx(), x))
    return _WELLS[name]


def replay_labels(name):
    """the 0-based labels of the used barcodes at the start of every iteration, replayed from the file's step log"""
    r = ref()
    _, _, labels, _ = well(name)
    lab = labels[labels > 0].astype(np.int64) - 1
    out = []
    steps = r[name + ".steps"]
    for it in range(1, int(r[name + ".counts"][3]) + 1):
        out.append(lab.copy())
        for s in steps[steps[:, 0] == it]:
            if s[5]:
                lab[lab == s[2]] = s[1]
                lab[lab > s[2]] -= 1
    return out


@pytest.mark.parametrize("name", sorted(M.FIXTURES))
def test_cluster_medians_equal_the_file_on_every_iteration(name):
    from cellranger_amd import engine as E

    r = ref()
    _, pca, labels, _ = well(name)
    sub = np.ascontiguousarray(pca[labels > 0])
    for i, lab in enumerate(replay_labels(name)):
        o = ctx().cluster_medians(sub, lab)
        want = r["%s.medoids.%d" % (name, i)]
        assert o["medians"].shape == want.shape and np.array_equal(o["medians"], want), (name, i)
        assert np.array_equal(o["sizes"], np.bincount(lab).astype(np.uint64))
        assert E.linkage_complete(o["medians"]).tobytes() == r["%s.Z.%d" % (name, i)].tobytes(), (name, i)


def test_cluster_medians_columns_and_strides():
    rs = np.random.RandomState(3)
    x = rs.normal(0, 1, (257, 7))
    lab = rs.randint(0, 3, 257)
    full = ctx().cluster_medians(x, lab)["medians"]
    assert np.array_equal(full, M.cluster_medians(x, lab, 3))
    assert np.array_equal(ctx().cluster_medians(x, lab, num_pcs=4)["medians"], full[:, :4])      # a view of the first columns: ld > d
    one = ctx().cluster_medians(x[:1], np.zeros(1, np.int32))["medians"]
    assert np.array_equal(one, x[:1])


@pytest.mark.parametrize("name", sorted(M.FIXTURES))
def test_merge_clusters_equals_the_file(name):
    from cellranger_amd import engine as E

    x, pca, labels, m = well(name)
    o = E.merge_clusters(ctx(), m, pca, labels, n_features=M.G)
    check_against_file(ref(), name, o)
    assert o["labels"].shape == labels.shape and np.array_equal(o["labels"] == 0, labels == 0)
    assert o["n_tests"] + o["n_skipped"] == len(o["steps"]) and o["n_clusters_out"] == o["n_clusters_in"] - o["n_merges"]
    assert all(o[k] >= 0.0 for k in ("plan_ms", "medians_ms", "linkage_ms", "pairs_ms", "total_ms"))


def test_an_error_of_a_pair_call_propagates():
    from cellranger_amd import _lib
    from cellranger_amd import engine as E

    x, pca, labels, _ = well("distinct")
    zero = x.copy()
    zero[:, 0] = 0      # a cell without counts in a cluster that is tested
    with pytest.raises(_lib.CrgpuError) as e:
        E.merge_clusters(ctx(), _matrix(ctx(), zero), pca, labels, n_features=M.G)
    assert e.value.code == -1 and "a cell without counts" in str(e.value)
    with pytest.raises(ValueError):
        E.merge_clusters(ctx(), well("distinct")[3], pca[:-1], labels, n_features=M.G)


def test_run_graph_clustering_with_and_without_the_merge():
    from cellranger_amd import engine as E

    x, pca, labels, m = well("oversplit")
    m.n_features = M.G

    def split_labels(row, col):      # stands for the binary: (node, community) pairs that give the over-split labels back
        return [(i, int(l) - 1) for i, l in enumerate(labels)]

    plain = E.run_graph_clustering(ctx(), pca, louvain=split_labels)
    assert sorted(plain) == sorted(["num_neighbors", "indices", "distances", "nn_indptr", "nn_indices", "nn_nodes", "nn_links", "nn_density",
                                    "pairs_evaluated", "fit_ms", "labels", "clusters"])
    assert np.array_equal(plain["labels"], labels)
    both = E.run_graph_clustering(ctx(), pca, louvain=split_labels, merge_matrix=m)
    assert sorted(set(both) - set(plain)) == ["merge", "merged_clusters", "merged_labels"]
    assert all(np.array_equal(both[k], plain[k]) for k in ("labels", "clusters", "indices", "nn_indices"))
    assert np.array_equal(both["merged_labels"], ref()["oversplit.labels"]) and both["merge"]["n_clusters_out"] == 3
    assert sorted(np.unique(both["merged_clusters"]).tolist()) == [1, 2, 3]
    assert "merge" not in E.run_graph_clustering(ctx(), pca, merge_matrix=m)      # without a louvain there are no labels to merge
