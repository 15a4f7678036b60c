"""GPU tests of the local sSeq comparison of two groups of cells (Context.sseq_pairs, SseqPairs.compare; csrc/sseq_pair.h).

THE CONTRACT: every output of a pair equals, byte for byte, what the existing entry points give on the same context for cluster 1 of
the sub-matrix select_barcodes_dev(m, cols), cols = the cells of groups_a in (group, cell) order, then those of groups_b, with the labels
1 .. 1, 2 .. 2 (Context.sseq_params + Context.sseq_diffexp, row 0).  Integers, use, the exact / asymptotic split and n_de also equal the
restatement (tests/merge_clusters_numpy.compare).

The matrix: G = 40, N = 300, six groups of 1, 30, 64, 20, 130 and 35 cells in shuffled cell order and 20 cells of group -1.  Gene 0 is
in every cell, gene 25 in none, gene 26 only in cells outside the pairs that are tested with it, the others run from 2 % to every cell.
Genes 1 .. 8, 9 .. 16 and 17 .. 24 have exactly 0, 1, 63, 64, 65, 127, 128 and 129 entries in side a of the pairs whose side a is one,
two and three groups: a lane of the row-sum kernel gets none, one or several entries, and a run ends on, before and after a multiple
of 64."""
import numpy as np
import pytest

import merge_clusters_numpy as M
from test_gpu_sseq import _matrix, ctx

pytestmark = pytest.mark.gpu
EINVAL = -1
G, N = 40, 300
SIZES = (1, 30, 64, 20, 130, 35)
LENGTHS = (0, 1, 63, 64, 65, 127, 128, 129)
SIDES_A = ([4], [1, 4], [0, 1, 4])      # genes 1 .. 8, 9 .. 16, 17 .. 24 are built on these
PAIRS = [([4], [2]), ([1, 4], [2, 5]), ([0, 1, 4], [2, 3, 5]), ([0], [5]), ([5], [0]), ([0], [1]), ([3], [1, 2]), ([2, 5], [0, 1]), ([0, 1, 2], [3, 4, 5]),
         ([1, 3, 5], [0, 2, 4])]
VECTORS = ("use", "mean", "phi_mm", "phi", "sums_a", "sums_b", "norm_mean_a", "norm_mean_b", "log2_fold_change", "p_values", "adjusted_p_values",
           "below_median")
SCALARS = ("zeta_hat", "delta", "n_used", "s_a", "s_b", "n_cells_a", "n_cells_b", "n_exact", "n_asymptotic", "n_terms", "n_de")
_STATE = {}


def well():
    """-> (x int64[G, N], groups i32[N])"""
    rs = np.random.RandomState(77)
    groups = np.concatenate([np.repeat(np.arange(6), SIZES), np.full(N - sum(SIZES), -1)]).astype(np.int32)
    rs.shuffle(groups)
    x = np.zeros((G, N), np.int64)
    x[0] = rs.randint(30, 70, N)                    # in every cell: no empty cell, and sums above 900 on both sides of the large pairs
    dens = np.concatenate([np.exp(rs.uniform(np.log(0.02), 0.0, 12)), [0.5]])
    for g, p in zip(list(range(27, 39)) + [39], dens):
        x[g] = rs.randint(1, 30, N) * (rs.rand(N) < p)
    x[38] = rs.randint(1, 9, N)                     # another one in every cell
    for s, side in enumerate(SIDES_A):
        cells = np.concatenate([np.flatnonzero(groups == k) for k in side])
        outside = np.setdiff1d(np.arange(N), cells)
        for j, n in enumerate(LENGTHS):
            g = 1 + 8 * s + j
            x[g, cells[:n]] = rs.randint(1, 40, n)
            x[g, outside] = rs.randint(1, 40, len(outside)) * (rs.rand(len(outside)) < 0.4)
    x[26, (groups == 3) | (groups == -1)] = rs.randint(1, 20, int(((groups == 3) | (groups == -1)).sum()))
    return x, groups


def state():
    if not _STATE:
        x, groups = well()
        m = _matrix(ctx(), x)
        _STATE.update(x=x, groups=groups, m=m, plan=ctx().sseq_pairs(m, groups, n_features=G), pairs={}, composed={})
    return _STATE


def pair(a, b):
    s = state()
    key = (tuple(a), tuple(b))
    if key not in s["pairs"]:
        s["pairs"][key] = s["plan"].compare(a, b)
    return s["pairs"][key]


def composed(a, b):
    """cluster 1 of the parent's path on the sub-matrix, under the names of the pair call"""
    s = state()
    key = (tuple(a), tuple(b))
    if key not in s["composed"]:
        cols, na = M.pair_columns(s["groups"], a, b)
        sub = ctx().select_barcodes_dev(s["m"], cols)
        params = ctx().sseq_params(sub, n_features=G)
        P = params.download()
        o = ctx().sseq_diffexp(sub, params, np.array([1] * na + [2] * (len(cols) - na), np.int32), 2)
        adj = o["adjusted_p_values"][0]
        s["composed"][key] = dict(use=P["use_g"].astype(np.uint8), mean=P["mean_g"], phi_mm=P["phi_mm_g"], phi=P["phi_g"], sums_a=o["sums_in"][0],
                                  sums_b=o["sums_out"][0], norm_mean_a=o["norm_mean_in"][0], norm_mean_b=o["norm_mean_out"][0],
                                  log2_fold_change=o["log2_fold_change"][0], p_values=o["p_values"][0], adjusted_p_values=adj,
                                  below_median=o["below_median"][0], zeta_hat=P["zeta_hat"], delta=P["delta"], n_used=P["n_used"], s_a=float(o["s_a"][0]),
                                  s_b=float(o["s_b"][0]), n_cells_a=na, n_cells_b=len(cols) - na, n_exact=int(o["n_exact"][0]),
                                  n_asymptotic=int(o["n_asymptotic"][0]), n_terms=o["n_terms"] // 2, n_terms_both=o["n_terms"],
                                  n_de=int(np.sum(adj < 0.05)))
        params.free()
    return s["composed"][key]


def bits(o):
    out = {k: np.ascontiguousarray(o[k]).tobytes() for k in VECTORS}
    out.update({k: np.float64(o[k]).tobytes() for k in SCALARS})
    return out


def test_the_well_has_the_run_lengths_it_is_for():
    x, groups = well()
    assert np.bincount(groups + 1).tolist() == [20] + list(SIZES) and not np.array_equal(np.sort(groups), groups)
    for s, side in enumerate(SIDES_A):
        cells, na = M.pair_columns(groups, side, [])
        assert [int((x[1 + 8 * s + j, cells] > 0).sum()) for j in range(8)] == list(LENGTHS) and na == len(cells)
    assert x.sum(axis=0).min() > 0 and x[25].sum() == 0 and np.all(x[0] > 0) and np.all(x[38] > 0)
    assert x[26].sum() > 0 and x[26, np.isin(groups, [0, 1, 2, 4, 5])].sum() == 0
    per_gene = (x > 0).mean(axis=1)
    assert per_gene.min() == 0.0 and per_gene.max() == 1.0 and np.sum((per_gene > 0.01) & (per_gene < 0.2)) >= 3


@pytest.mark.parametrize("a,b", PAIRS)
def test_pair_equals_the_composed_path_byte_for_byte(a, b):
    got, want = pair(a, b), composed(a, b)
    gb, wb = bits(got), bits(want)
    assert gb == wb, [k for k in gb if gb[k] != wb[k]]
    assert 2 * got["n_terms"] == want["n_terms_both"] and got["n_runs"] == len(a) + len(b)
    # the restatement: integers, use, the split and n_de
    s = state()
    r = M.compare(s["x"], s["groups"], a, b)
    assert np.array_equal(got["use"] != 0, r["use"]) and got["n_used"] == r["n_used"]
    assert np.array_equal(got["sums_a"], r["sums_a"]) and np.array_equal(got["sums_b"], r["sums_b"])
    assert np.array_equal(got["below_median"] == 255, r["below_median"] == 255)
    assert (got["n_exact"], got["n_asymptotic"], got["n_terms"], got["n_cells_a"], got["n_cells_b"]) == (
        r["n_exact"], r["n_asymptotic"], r["n_terms"], r["n_cells_a"], r["n_cells_b"])
    assert np.all(np.abs(r["adjusted_p_values"] - 0.05) > 1e-6 * 0.05) and got["n_de"] == r["n_de"]
    assert np.all(got["p_values"][got["use"] == 0] == 1.0) and np.all(np.isnan(got["phi"]) == (got["use"] == 0))
    assert not got["use"][25] and got["sums_a"][25] == got["sums_b"][25] == 0


def test_both_kinds_of_test_and_the_gene_outside_the_pair_occur():
    big = pair([0, 1, 4], [2, 3, 5])
    assert big["n_asymptotic"] >= 2 and big["n_exact"] >= 20
    assert pair([0], [5])["n_asymptotic"] == 0
    out = pair([4], [2])      # gene 26 lives in group 3 and the cells of no group alone
    assert out["sums_a"][26] == out["sums_b"][26] == 0 and not out["use"][26]
    assert pair([3], [1, 2])["sums_a"][26] > 0
    assert any(pair(a, b)["n_de"] > 0 for a, b in PAIRS) and any(pair(a, b)["n_de"] < G for a, b in PAIRS)


def test_the_pair_of_all_groups_equals_the_parameters_of_the_permuted_matrix():
    s = state()
    cols, na = M.pair_columns(s["groups"], [0, 1, 2], [3, 4, 5])
    assert len(cols) == sum(SIZES)
    params = ctx().sseq_params(ctx().select_barcodes_dev(s["m"], cols), n_features=G)
    P = params.download()
    got = pair([0, 1, 2], [3, 4, 5])
    for k, pk in (("mean", "mean_g"), ("phi_mm", "phi_mm_g"), ("phi", "phi_g")):
        assert got[k].tobytes() == P[pk].tobytes(), k
    assert np.array_equal(got["use"] != 0, P["use_g"]) and (got["zeta_hat"], got["delta"], got["n_used"]) == (P["zeta_hat"], P["delta"], P["n_used"])
    params.free()


def test_two_runs_two_plans_and_the_class_thresholds_move_no_bit():
    s = state()
    again = ctx().sseq_pairs(s["m"], s["groups"], n_features=G)
    for a, b in (([0, 1, 4], [2, 3, 5]), ([5], [0]), ([1, 4], [2, 5])):
        first = bits(pair(a, b))
        assert bits(s["plan"].compare(a, b)) == first and bits(again.compare(a, b)) == first
        for kw in (dict(wave_min=1, wg_min=0xFFFFFFFF), dict(wave_min=1, wg_min=1), dict(wave_min=5, wg_min=64)):
            assert bits(s["plan"].compare(a, b, **kw)) == first, kw
        slim = s["plan"].compare(a, b, vectors=False)      # no vector asked for: the scalars are the same
        assert all(np.float64(slim[k]).tobytes() == first[k] for k in SCALARS) and "p_values" not in slim
    again.free()


def test_de_threshold():
    a, b = [1, 4], [2, 5]
    q = pair(a, b)["adjusted_p_values"]
    plan = state()["plan"]
    assert pair(a, b)["n_de"] == int(np.sum(q < 0.05)) == plan.compare(a, b, de_threshold=0.05)["n_de"]
    for thr in (1e-30, 0.5, 1.0, 2.0):
        assert plan.compare(a, b, de_threshold=thr)["n_de"] == int(np.sum(q < thr)), thr


def _refused(fn, *words):
    from cellranger_amd import _lib

    with pytest.raises(_lib.CrgpuError) as e:
        fn()
    assert e.value.code == EINVAL
    for w in words:
        assert w in str(e.value), (w, str(e.value))


def test_refusals_with_their_messages():
    s = state()
    c, m, groups, plan = ctx(), s["m"], s["groups"], s["plan"]
    first = bits(pair([1, 4], [2, 5]))
    _refused(lambda: c.sseq_pairs(m, groups, n_features=2), "2 features, at least 3")
    _refused(lambda: c.sseq_pairs(m, groups, n_features=G - 1), "a row >= n_features (39)")
    _refused(lambda: c.sseq_pairs(m, groups, n_groups=7, n_features=G), "group 6 is empty")
    _refused(lambda: c.sseq_pairs(m, groups, n_groups=5, n_features=G), "group 5 of cell", "-1 to 4")
    _refused(lambda: c.sseq_pairs(m, np.where(groups == -1, -2, groups), n_features=G), "group -2 of cell")
    _refused(lambda: c.sseq_pairs(m, np.where(groups > 0, 0, groups), n_groups=1, n_features=G), "1 groups, 2 to")
    _refused(lambda: c.sseq_pairs(m, np.where(groups == 3, 4, groups), n_features=G), "group 3 is empty")
    _refused(lambda: plan.compare([], [1]), "groups_a is empty")
    _refused(lambda: plan.compare([1], []), "groups_b is empty")
    _refused(lambda: plan.compare([2, 1], [3]), "groups_a must be strictly ascending")
    _refused(lambda: plan.compare([0], [3, 3]), "groups_b must be strictly ascending")
    _refused(lambda: plan.compare([0, 2], [1, 2, 3]), "group 2 is on both sides")
    _refused(lambda: plan.compare([0], [6]), "group 6 of groups_b", "6 groups")
    _refused(lambda: plan.compare([0], [1], de_threshold=-0.5), "de_threshold")
    bad = plan.n_features
    plan.n_features = G + 1
    try:
        _refused(lambda: plan.compare([0], [1], vectors=False), "the plan has 40 features")
    finally:
        plan.n_features = bad
    # a cell without counts is refused for the pairs that hold it, and no gene that varies for two equal cells
    x = s["x"][:, :12].copy()
    x[:, 5] = 0
    x[:, 7] = x[:, 6]
    g = np.array([0, 0, 0, 1, 1, 2, 3, 4, 0, 1, 1, 0], np.int32)
    small = c.sseq_pairs(_matrix(c, x), g, n_features=G)
    _refused(lambda: small.compare([0], [2]), "a cell without counts")
    _refused(lambda: small.compare([3], [4]), "no gene varies over the cells")
    ok = small.compare([0], [1])
    assert ok["n_cells_a"] == 5 and ok["n_cells_b"] == 4
    small.free()
    assert bits(plan.compare([1, 4], [2, 5])) == first      # the context and the plan are still good
