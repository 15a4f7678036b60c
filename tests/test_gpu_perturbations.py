"""GPU tests of the MEASURE_PERTURBATIONS stage (SseqPairs.bootstrap, engine.measure_perturbations; csrc/perturbations.h) against the
restatement tests/perturbations_numpy.py.

The well: G = 40 genes, N = 400 cells in shuffled order.  130 control cells (100 with one Non-Targeting guide, 30 with two), the
perturbations T2 (9 cells: skipped), T5 (10), T12 (64), T30 (100), the multi-target perturbation T5|T12 (20 cells with the guides of
both; the clusters are numbered by the sorted target IDS, so it stands between T5 and T12), TX (15 cells; its target id is not a row of
the matrix: tested, but without a fold change) and 52 cells without a call.  Gene 0 has a count in every cell; a target's counts are
lowered in its perturbed cells.

The bootstrap sums are integers and must equal the restatement exactly.  The pair vectors must be byte-equal to SseqPairs.compare on a
plan of the two groups alone.  The CI bounds come from log2 and a percentile in f64 on both sides: their tolerance is derived beside
the check."""
import numpy as np
import pytest

import perturbations_numpy as P
from test_gpu_sseq import _matrix, ctx

pytestmark = pytest.mark.gpu
EINVAL = -1
G, N, B, SEED = 40, 400, 500, 20240607
GENE_IDS = ["ENSG%011d" % g for g in range(G)]
GENE_NAMES = ["Gene%02d" % (G - g) for g in range(G)]      # names in another order than the ids
FEATURE_REF = [dict(id="NT1", target_gene_id="Non-Targeting", target_gene_name="Non-Targeting"),
               dict(id="NT2", target_gene_id="Non-Targeting", target_gene_name="Non-Targeting"),
               dict(id="GA", target_gene_id=GENE_IDS[5], target_gene_name="T5"),
               dict(id="GB", target_gene_id=GENE_IDS[12], target_gene_name="T12"),
               dict(id="GC", target_gene_id=GENE_IDS[30], target_gene_name="T30"),
               dict(id="GD", target_gene_id=GENE_IDS[2], target_gene_name="T2"),
               dict(id="GX", target_gene_id="ENSG_ABSENT", target_gene_name="TX")]
CELLS = (("NT1", 1, 100), ("NT1|NT2", 2, 30), ("GD", 1, 9), ("GA", 1, 10), ("GB", 1, 64), ("GC", 1, 100), ("GB|GA", 2, 20), ("GX", 1, 15), (None, 0, 52))
_STATE = {}


def well():
    """-> (x int64[G, N], barcodes, calls)"""
    rs = np.random.RandomState(404)
    kind = np.concatenate([np.full(n, i) for i, (_, _, n) in enumerate(CELLS)])
    rs.shuffle(kind)
    barcodes = ["BC%04d-1" % i for i in range(N)]
    calls = {barcodes[i]: (CELLS[k][0], CELLS[k][1]) for i, k in enumerate(kind) if CELLS[k][0] is not None}
    x = rs.poisson(np.exp(rs.uniform(np.log(0.05), np.log(12.0), G))[:, None], (G, N))
    x[0] = rs.randint(20, 60, N)      # no empty cell
    for guides, gene in (("GA", 5), ("GB", 12), ("GC", 30), ("GB|GA", 5), ("GB|GA", 12)):
        hit = np.array([CELLS[k][0] == guides for k in kind])
        x[gene] = np.where(hit, rs.binomial(x[gene] + 2, 0.25), x[gene] + 2)
    return x.astype(np.int64), barcodes, calls


def state():
    if not _STATE:
        x, barcodes, calls = well()
        per_bc, names = P.clusters(FEATURE_REF, calls, barcodes)
        _STATE.update(x=x, barcodes=barcodes, calls=calls, per_bc=per_bc, names=names, m=_matrix(ctx(), x))
    return _STATE


def two_group_compare(cells_a, cells_b):
    """SseqPairs.compare on a plan that holds these two groups alone"""
    s = state()
    groups = np.full(N, -1, np.int32)
    groups[cells_a], groups[cells_b] = 0, 1
    plan = ctx().sseq_pairs(s["m"], groups, n_features=G)
    try:
        return plan.compare([0], [1])
    finally:
        plan.free()


def stage():
    from cellranger_amd import engine as E

    s = state()
    if "got" not in s:
        s["got"] = E.measure_perturbations(ctx(), s["m"], GENE_IDS, GENE_NAMES, FEATURE_REF, s["calls"], s["barcodes"], num_bootstraps=B, seed=SEED)
        s["want"] = P.measure(s["x"], GENE_IDS, GENE_NAMES, FEATURE_REF, s["calls"], s["barcodes"], two_group_compare, B=B, seed=SEED)
    return s["got"], s["want"]


def grouped_plan():
    """the plan of the stage's grouping: the tested perturbations in cluster order, then the control"""
    s = state()
    if "plan" not in s:
        tested = [c for c in sorted(s["names"]) if s["names"][c] in ("T5", "T5|T12", "T12", "T30", "TX")]
        groups = np.full(N, -1, np.int32)
        for j, c in enumerate(tested):
            groups[s["per_bc"] == c] = j
        control = [c for c, n in s["names"].items() if n == "Non-Targeting"][0]
        groups[s["per_bc"] == control] = len(tested)
        s.update(groups=groups, plan=ctx().sseq_pairs(s["m"], groups, n_features=G), control_group=len(tested))
    return s["plan"], s["groups"], s["control_group"]


# (gene, group_a, group_b, stream); the groups: 0 = T5, 1 = T5|T12, 2 = T12, 3 = T30, 4 = TX, 5 = the control.  The first five are the stage's
ITEMS = [(5, 0, 5, 0), (5, 1, 5, 1), (12, 1, 5, 2), (12, 2, 5, 3), (30, 3, 5, 4), (0, 5, 2, 9), (12, 4, 0, 7), (39, 1, 3, 2)]


def want_sums(items, n_bootstraps=B, seed=SEED):
    s = state()
    _, groups, _ = grouped_plan()
    cache = s.setdefault("sums", {})
    for it in items:
        if (it, n_bootstraps, seed) not in cache:
            g, ka, kb, stream = it
            cache[(it, n_bootstraps, seed)] = (P.bootstrap_sums(s["x"][g, np.flatnonzero(groups == ka)], seed, stream, 0, n_bootstraps),
                                               P.bootstrap_sums(s["x"][g, np.flatnonzero(groups == kb)], seed, stream, 1, n_bootstraps))
    return (np.stack([cache[(it, n_bootstraps, seed)][0] for it in items]), np.stack([cache[(it, n_bootstraps, seed)][1] for it in items]))


def test_the_well_is_what_it_is_for():
    s = state()
    sizes = {s["names"][c]: int((s["per_bc"] == c).sum()) for c in s["names"]}
    assert sizes == {"Non-Targeting": 130, "None": 52, "T12": 64, "T5|T12": 20, "T2": 9, "T30": 100, "T5": 10, "TX": 15}
    assert s["x"].sum(axis=0).min() > 0 and not np.array_equal(np.sort(s["per_bc"]), s["per_bc"])
    _, groups, control = grouped_plan()
    assert control == 5 and np.bincount(groups + 1).tolist() == [61, 10, 20, 64, 100, 15, 130]


def test_bootstrap_equals_the_restatement():
    plan, _, _ = grouped_plan()
    sa, sb = plan.bootstrap(ITEMS, n_bootstraps=B, seed=SEED)
    wa, wb = want_sums(ITEMS)
    assert sa.shape == sb.shape == (len(ITEMS), B) and sa.dtype == np.uint64
    assert np.array_equal(sa, wa) and np.array_equal(sb, wb)
    # items 0 and 1 share the control column of gene 5, 2 and 3 that of gene 12: another stream, other draws
    assert not np.array_equal(sb[0], sb[1]) and not np.array_equal(sb[2], sb[3])
    assert sa[:5].std(axis=1).min() > 0 and sb[:5].std(axis=1).min() > 0


def test_batch_order_paths_and_chunks_move_no_value():
    plan, _, _ = grouped_plan()
    wa, wb = want_sums(ITEMS)
    order = [6, 2, 7, 0, 5, 3, 1, 4]
    sa, sb = plan.bootstrap([ITEMS[i] for i in order], n_bootstraps=B, seed=SEED)
    assert np.array_equal(sa, wa[order]) and np.array_equal(sb, wb[order])
    one_a, one_b = plan.bootstrap([ITEMS[3]], n_bootstraps=B, seed=SEED)      # alone in its batch
    assert np.array_equal(one_a[0], wa[3]) and np.array_equal(one_b[0], wb[3])
    for kw in (dict(lds_cells=1), dict(lds_cells=100), dict(draws_per_wg=1), dict(draws_per_wg=3), dict(draws_per_wg=500), dict(lds_cells=40960, draws_per_wg=7)):
        sa, sb = plan.bootstrap(ITEMS, n_bootstraps=B, seed=SEED, **kw)
        assert np.array_equal(sa, wa) and np.array_equal(sb, wb), kw
    # the default B, another seed, a small B
    da, db = plan.bootstrap(ITEMS[:2], n_bootstraps=0, seed=SEED)
    assert np.array_equal(da, wa[:2]) and np.array_equal(db, wb[:2])
    ta, tb = plan.bootstrap(ITEMS[:2], n_bootstraps=3, seed=SEED + 1)
    xa, xb = want_sums(ITEMS[:2], 3, SEED + 1)
    assert np.array_equal(ta, xa) and np.array_equal(tb, xb) and not np.array_equal(ta, wa[:2, :3])


def _refused(fn, *words):
    from cellranger_amd import _lib

    with pytest.raises(_lib.CrgpuError) as e:
        fn()
    assert e.value.code == EINVAL
    for w in words:
        assert w in str(e.value), (w, str(e.value))


def test_refusals_with_their_messages():
    plan, _, _ = grouped_plan()
    _refused(lambda: plan.bootstrap(np.zeros((0, 4), np.uint32)))
    _refused(lambda: plan.bootstrap([(G, 0, 5, 0)]), "gene 40 of item 0", "40 features")
    _refused(lambda: plan.bootstrap([(0, 0, 5, 0), (0, 6, 5, 0)]), "groups 6 and 5 of item 1", "6 groups")
    _refused(lambda: plan.bootstrap([(0, 0, 6, 0)]), "groups 0 and 6 of item 0")
    _refused(lambda: plan.bootstrap([(0, 2, 2, 0)]), "group 2 is on both sides of item 0")
    _refused(lambda: plan.bootstrap([(0, 0, 5, 0)], n_bootstraps=65537), "65537 bootstraps, at most 65536")
    _refused(lambda: plan.bootstrap([(0, 0, 5, 0)], lds_cells=40961), "lds_cells 40961", "40960")
    sa, sb = plan.bootstrap(ITEMS[:1], n_bootstraps=B, seed=SEED)      # the context and the plan are still good
    wa, wb = want_sums(ITEMS[:1])
    assert np.array_equal(sa, wa) and np.array_equal(sb, wb)


def test_stage_integers_names_and_tables_equal_the_restatement():
    got, want = stage()
    assert want["names"] == ["T5", "T5|T12", "T12", "T30", "TX"] and want["skipped"] == ["T2"]
    assert got["cluster_names"] == want["names"] and list(got["results_per_perturbation"]) == want["names"]
    assert got["num_cells_per_perturbation"] == want["num_cells_per_perturbation"]
    assert np.array_equal(got["cluster_per_bc"], want["cluster_per_bc"]) and got["perturbation_keys"] == want["perturbation_keys"]
    # targets: the multi-target perturbation has two, TX (a target id that is no row of the matrix) has none
    assert {k: list(v) for k, v in got["log2_fold_change"].items()} == {"T5": ["T5"], "T5|T12": ["T5", "T12"], "T12": ["T12"], "T30": ["T30"], "TX": []}
    assert {k: list(v) for k, v in got["log2_fold_change"].items()} == {k: list(v) for k, v in want["log2_fold_change"].items()}
    assert got["items"] == ITEMS[:5]
    assert got["results_all_perturbations"].shape == want["results_all_perturbations"].shape == (G, 15)
    assert got["results_all_perturbations"].tobytes() == want["results_all_perturbations"].tobytes()
    # the summary: names, order of the rows, integers; the unadjusted p value
    assert got["summary_columns"] == want["summary_columns"] and got["summary_columns"][1] == "Target Gene" and len(got["summary"]) == 5
    for g, w in zip(got["summary"], want["summary"]):
        assert g[:4] == w[:4] and g[6:] == w[6:], (g, w)
    assert [r[2] for r in got["summary"]] == sorted(r[2] for r in got["summary"])
    name, target = got["summary"][0][:2]
    r = got["results_per_perturbation"][name]
    gene = GENE_IDS.index({"T5": GENE_IDS[5], "T12": GENE_IDS[12], "T30": GENE_IDS[30]}[target])
    assert got["summary"][0][3] == r["p_values"][gene] and got["summary"][0][7] == r["sums_a"][gene] / r["n_cells_a"] and got["summary"][0][8] == 130
    assert all(row[2] < 0 for row in got["summary"])      # every target is knocked down in this well
    assert got["top_perturbed_genes"] == want["top_perturbed_genes"] and all(1 <= len(v) <= 10 for v in got["top_perturbed_genes"].values())
    for k in ("plan_ms", "pairs_ms", "bootstrap_ms", "ci_ms", "total_ms"):
        assert got[k] >= 0.0


def test_stage_pairs_are_byte_equal_to_compare():
    got, want = stage()
    for name in want["names"]:
        g, w = got["results_per_perturbation"][name], want["results_per_perturbation"][name]
        for k, _ in type(grouped_plan()[0]).VECTORS:
            assert g[k].tobytes() == w[k].tobytes(), (name, k)
        for k in ("zeta_hat", "delta", "s_a", "s_b", "n_cells_a", "n_cells_b", "n_exact", "n_asymptotic", "n_de", "n_used"):
            assert np.float64(g[k]).tobytes() == np.float64(w[k]).tobytes(), (name, k)
        for t, res in got["log2_fold_change"][name].items():
            assert res == want["log2_fold_change"][name][t]


def test_stage_ci_bounds():
    """The restatement computes log2((1 + A) / (1 + s_a)) - log2((1 + B) / (1 + s_b)) per draw with numpy and takes np.percentile; the
    library computes the same expression with the C library's log2 and cr_quantile_sorted.  With M = max(1, |t_a|, |t_b|) over the
    draws (t_a, t_b the two log terms) the bound 2^-50 M is four units of 2^-52 M, and the two computations can differ by:
      the two divisions     correctly rounded on both sides from equal operands: nothing;
      the two log2          each side within one ulp of the value, so the sides differ by at most ulp(t) <= 2^-52 M per term;
      the subtraction       correctly rounded on both sides: it passes on the operands' differences, at most 2 x 2^-52 M, and, where
                            they land on different sides of a rounding boundary, one ulp of the result (|fc| <= 2 M: 2^-52 x 2 M / 2);
      the percentile        an order statistic moves by no more than its inputs do; cr_lerp is numpy's _lerp operation for operation
                            (a difference, a product with t in [0, 1], a sum), each correctly rounded, passing differences on with a
                            factor of at most 1 and adding at most one rounding of the result, 2^-53 x 2 M.
    Together at most (2 + 1 + 1) x 2^-52 M = 2^-50 M.  The figures are printed before the assertion.
    The library's own CI on the restatement's sums must be the stage's bit for bit: that pins the stage's sums to the restatement's."""
    from cellranger_amd import engine as E

    got, want = stage()
    n = 0
    for name in want["names"]:
        s_a, s_b = got["results_per_perturbation"][name]["s_a"], got["results_per_perturbation"][name]["s_b"]
        for target, (wlo, whi, sa, sb) in want["log2_fold_change_ci"][name].items():
            lo, hi = got["log2_fold_change_ci"][name][target]
            ta, tb = P.log_terms(sa, sb, s_a, s_b)
            tol = 2.0 ** -50 * max(1.0, np.abs(ta).max(), np.abs(tb).max())
            print("%s / %s: CI (%.6f, %.6f), |device - restatement| = %.3g, %.3g, bound %.3g" % (name, target, lo, hi, abs(lo - wlo), abs(hi - whi), tol))
            assert abs(lo - wlo) <= tol and abs(hi - whi) <= tol
            assert (lo, hi) == E.perturbation_ci(sa, sb, s_a, s_b)[:2]
            assert lo < hi and lo < got["log2_fold_change"][name][target][0] + 1.5 and hi > got["log2_fold_change"][name][target][0] - 1.5
            n += 1
    assert n == 5


def test_stage_returns_none_where_the_reference_does_and_by_feature_runs():
    from cellranger_amd import engine as E

    s = state()
    args = (ctx(), s["m"], GENE_IDS, GENE_NAMES)
    assert E.measure_perturbations(*args, [r for r in FEATURE_REF if r["target_gene_id"] != "Non-Targeting"], s["calls"], s["barcodes"]) is None
    assert E.measure_perturbations(*args, [dict(id=r["id"]) for r in FEATURE_REF], s["calls"], s["barcodes"]) is None
    no_control = {b: c for b, c in s["calls"].items() if not c[0].startswith("NT")}
    assert E.measure_perturbations(*args, FEATURE_REF, no_control, s["barcodes"]) is None
    by_feature = E.measure_perturbations(*args, FEATURE_REF, s["calls"], s["barcodes"], by_feature=True, num_bootstraps=50, seed=1)
    assert by_feature["cluster_names"] == ["GA", "GB", "GB|GA", "GC", "GX"] and by_feature["summary_columns"][1] == "Target Guide"
    assert list(by_feature["log2_fold_change"]["GB|GA"]) == ["GB", "GA"] and by_feature["num_cells_per_perturbation"]["Ignore"] == 52
    ignoring = E.measure_perturbations(*args, FEATURE_REF, s["calls"], s["barcodes"], ignore_multiples=True, num_bootstraps=50, seed=1)
    assert ignoring["cluster_names"] == ["T5", "T12", "T30", "TX"] and ignoring["num_cells_per_perturbation"]["Ignore"] == 50
    assert ignoring["num_cells_per_perturbation"]["Non-Targeting"] == 100


def test_csv_writers(tmp_path):
    import csv

    from cellranger_amd import engine as E

    got, _ = stage()
    E.write_perturbation_efficiencies_csv(tmp_path / "perturbation_efficiencies.csv", got)
    E.write_transcriptome_analysis_csv(tmp_path / "transcriptome_analysis.csv", got, GENE_IDS, GENE_NAMES)
    E.write_top_perturbed_genes_csv(tmp_path / "top_perturbed_genes.csv", got)
    rows = list(csv.reader(open(tmp_path / "perturbation_efficiencies.csv")))
    assert rows[0] == got["summary_columns"] and len(rows) == 6 and rows[1][0] == got["summary"][0][0] and float(rows[1][2]) == got["summary"][0][2]
    rows = list(csv.reader(open(tmp_path / "transcriptome_analysis.csv")))
    assert rows[0] == E.differential_expression_header(5, got["cluster_names"]) and rows[0][2] == "Perturbation T5, Mean Counts"
    assert len(rows) == G + 1 and rows[1][:2] == [GENE_IDS[0], GENE_NAMES[0]] and float(rows[13][3]) == got["results_all_perturbations"][12, 1]
    rows = list(csv.reader(open(tmp_path / "top_perturbed_genes.csv")))
    assert rows[0][:4] == ["Perturbation: T5, Gene Name", "Perturbation: T5, Gene ID", "Perturbation: T5, Log2 Fold Change", "Perturbation: T5, Adjusted p-value"]
    assert len(rows[0]) == 20 and 2 <= len(rows) <= 11
