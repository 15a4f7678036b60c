"""GPU tests of the marginal caller (Context.marginal_calls / tag_moments, engine.call_protospacers / call_antibodies /
call_tags_marginal; csrc/marginal_calls.h).

Expected values: tests/golden/marginal_calls_reference.npz (the reference's own calls and scikit-learn 1.7.2's fitted parameters;
tests/test_marginal_calls_restatement.py says how they were recorded) and the histogram-order restatement of
tests/marginal_calls_numpy.py, computed once per fixture and shared.  Equal: status, calls, cells_assigned, umi_threshold_observed,
total UMIs, the number of distinct values, the winner and its iteration count -- the recorder rejected fixtures whose integers hang on
the last bits, and the synthetic rows built here pass the same rule (marginal_calls_numpy.margins_ok) before they are used.  Weights,
means and the tied covariance: within 16 x `movement` of the file, absolutely (the factor the RPU fit uses for the same arithmetic;
movement = what a change of the summation order does to the restatement), against the golden file and against the restatement.
Bit for bit: run against run, CRGPU_MC_LDS_VALUES = 0 / 8 / default, a row alone against the same row among 69 others.

Measured on an MI355X, all fixtures: the largest distances (weights, means, covariance) are in the docstring of
test_fixtures_equal_the_reference_and_the_restatement."""
import numpy as np
import pytest

import jibes_numpy as JR
import marginal_calls_numpy as R
from test_marginal_calls_restatement import check_against_golden, distances, fixture_names, fixture_row, golden, parameters, restated

pytestmark = pytest.mark.gpu
EINVAL, ERANGE = -1, -6
FACTOR = 16.0
_WORST = {"golden": np.zeros(3), "restatement": np.zeros(3)}


def _matrix(dense_by_column, n_features):
    """a fresh context and its MatrixDev of V columns (the k-th whitelist entry each) from a dense V x n_features table"""
    import gpu_helpers as G

    c = G.fresh_ctx()
    V = len(dense_by_column)
    c.set_whitelist(0, np.arange(max(4096, V), dtype=np.uint32), length=16)
    seen = np.zeros(c.n_canon, np.uint32)
    seen[:V] = 1
    c.set_counts(0, 0, seen)
    cols, rows = np.nonzero(dense_by_column)
    m = c.assemble_matrix_dev(c.upload(cols.astype(np.uint32)), c.upload(rows.astype(np.uint32)), c.upload(dense_by_column[cols, rows].astype(np.uint32)),
                              len(cols))
    assert m.n_barcodes == V
    return c, m


def _interleave(rows_dense, seed, empty_column=None):
    """the given feature rows (each i64[V]) among GEX rows: -> (dense V x NF, the listed rows, not contiguous)"""
    rng = np.random.RandomState(seed)
    k, V = len(rows_dense), len(rows_dense[0])
    listed = np.cumsum(rng.randint(1, 4, k)) + 1            # 1 .. 3 gene rows between two listed rows, two in front
    NF = int(listed[-1]) + 3
    dense = rng.poisson(0.7, (V, NF)).astype(np.int64)
    for j, r in enumerate(rows_dense):
        dense[:, listed[j]] = r
    if empty_column is not None:
        dense[empty_column, :] = 0
    return dense, listed.astype(np.uint32)


def _row_fields(mc, p):
    return {k: mc.per_feature[k][p] for k in mc.per_feature}


def _got(mc, p):
    f = _row_fields(mc, p)
    return dict(fitted=bool(f["status"]), n_iter=int(f["n_iter"]), winner=int(f["winner"]), cells_assigned=int(f["cells_assigned"]),
                umi_threshold_observed=int(f["umi_threshold_observed"]), weight_low=f["weight_low"], weight_high=f["weight_high"],
                mean_low=f["mean_low"], mean_high=f["mean_high"], covariance=f["covariance"])


def _same_as_restatement(name, got, ref, called, ref_cols, bound):
    assert got["fitted"] == bool(ref["fitted"]), name
    assert np.array_equal(called, ref_cols), name
    assert got["cells_assigned"] == ref["cells_assigned"] and got["umi_threshold_observed"] == ref["umi_threshold_observed"], name
    if not ref["fitted"]:
        assert got["winner"] == 0xFFFFFFFF and got["n_iter"] == 0
        return np.zeros(3)
    assert (got["winner"], got["n_iter"]) == (ref["winner"], ref["n_iter"]), (name, got["winner"], got["n_iter"], ref["winner"], ref["n_iter"])
    d = distances(parameters(got), parameters(ref))
    print(name, "device - restatement (weights, means, covariance)", d, "bound", bound)
    assert np.all(d <= bound), (name, d, bound)
    return d


@pytest.mark.parametrize("V", [2, 3, 65, 257, 5000])
def test_fixtures_equal_the_reference_and_the_restatement(V):
    """Measured on an MI355X over all fixtures (bound: 16 x movement = 5.8e-13, 7.0e-13, 1.1e-12): see DESIGN.md, Marginal calls."""
    g = golden()
    bound = FACTOR * g["movement"]
    for thr in (1, 3):
        idx = [i for i in range(len(g["names"])) if int(g["V"][i]) == V and int(g["umi_threshold"][i]) == thr]
        if not idx:
            continue
        rows = [fixture_row(i)[4] for i in idx]
        dense, listed = _interleave(rows, 100 + V + thr)
        c, m = _matrix(dense, dense.shape[1])
        mc = c.marginal_calls(m, listed, umi_threshold=thr, n_features=dense.shape[1], want_histograms=True)
        per_cell = mc.cells_per_feature()
        fpc = np.zeros(V, np.int64)
        for p, i in enumerate(idx):
            name = fixture_names()[i]
            got, ref = _got(mc, p), restated(i)
            _, cols, vals, _, dn = fixture_row(i)
            _WORST["golden"] = np.maximum(_WORST["golden"], check_against_golden(i, got, per_cell[p].astype(np.int64), bound))
            _WORST["restatement"] = np.maximum(_WORST["restatement"], _same_as_restatement(name, got, ref, per_cell[p].astype(np.int64), cols[ref["calls"]], bound))
            f = _row_fields(mc, p)
            assert int(f["total_umis"]) == int(dn.sum())
            hv, hm = mc.histogram(p)
            want_v, want_m = R.row_histogram(V, cols, vals)
            assert int(f["n_distinct"]) == len(want_v) and np.array_equal(hv, want_v) and np.array_equal(hm, want_m), name
            fpc[per_cell[p]] += 1
        assert np.array_equal(mc.features_per_cell, fpc)
        listed_umis = dense[:, listed].sum(1)
        assert (mc.cells_with_0, mc.cells_with_1, mc.cells_with_many) == (int((fpc == 0).sum()), int((fpc == 1).sum()), int((fpc > 1).sum()))
        assert mc.cells_without_umis == int((listed_umis == 0).sum())
        md = mc.metadata()
        assert md["num_cells"] == V and md["num_singlets"] == mc.cells_with_1 and md["num_cells_without_features"] == mc.cells_with_0
        mc.free()
        m.free()
        c.close()
    print("largest distances so far: to the golden file", _WORST["golden"], "to the restatement", _WORST["restatement"], "bound", bound)


def _guarded(gen, seed, thr):
    """a synthetic row that passes the recorder's rejection rule (the next seed where one does not), with its restatement"""
    for s in range(seed, seed + 50):
        counts = np.asarray(gen(np.random.RandomState(s)), np.int64)
        cols = np.flatnonzero(counts)
        ref = R.fit_histogram(len(counts), cols, counts[cols], thr)
        if not ref["fitted"] or R.margins_ok(ref, np.unique(np.log10(1 + counts))):
            return counts, cols, ref
    raise AssertionError("no acceptable row")


def _synthetic_rows(V, n, thr, empty=None):
    def guide(rng):
        c = rng.poisson(0.03, V)
        k = rng.rand(V) < rng.uniform(0.02, 0.3)
        c[k] += rng.negative_binomial(3, 0.06, k.sum())
        return c

    def tag(rng):
        c = rng.poisson(2.0, V)
        k = rng.rand(V) < 0.2
        c[k] += rng.poisson(300, k.sum())
        return c

    def block_at_end(rng):      # leading zeros: a trial draw can land before the first entry
        c = np.zeros(V, np.int64)
        c[int(0.6 * V):] = 1 + rng.poisson(20, V - int(0.6 * V))
        return c

    def block_at_start(rng):    # trailing zeros: a trial draw can land behind the last entry
        c = np.zeros(V, np.int64)
        c[:int(0.4 * V)] = 1 + rng.poisson(20, int(0.4 * V))
        return c

    special = [lambda rng: np.zeros(V, np.int64),                                    # no entry
               lambda rng: np.where(np.arange(V) == V // 2, 9, 0),                   # one entry
               lambda rng: 1 + rng.poisson(5.0, V),                                  # no zeros
               lambda rng: np.where(rng.rand(V) < 0.25, 4, 0),                       # one distinct non-zero value
               lambda rng: np.full(V, 6),                                            # one distinct value over all cells
               block_at_end, block_at_start, tag]
    gens = (special + [guide] * n)[:n] if n >= 3 else [guide, tag][:n]
    def emptied(gen):      # an empty column of the well is a zero in every row
        def f(rng):
            c = np.array(gen(rng), np.int64)
            if empty is not None:
                c[empty] = 0
            return c
        return f

    return [_guarded(emptied(gen), 7000 + 50 * j, thr) for j, gen in enumerate(gens)]


_SEVENTY = {}


def _seventy():
    """the 70-row well at V = 257, fitted once: (rows, call result as plain arrays)"""
    if not _SEVENTY:
        V, thr = 257, 3
        rows = _synthetic_rows(V, 70, thr, empty=11)
        dense, listed = _interleave([r[0] for r in rows], 5, empty_column=11)
        c, m = _matrix(dense, dense.shape[1])
        mc = c.marginal_calls(m, listed, umi_threshold=thr, n_features=dense.shape[1])
        _SEVENTY.update(rows=rows, dense=dense, listed=listed, per_feature={k: v.copy() for k, v in mc.per_feature.items()}, cells=mc.cells_per_feature(),
                        fpc=mc.features_per_cell, tallies=(mc.cells_with_0, mc.cells_with_1, mc.cells_with_many, mc.cells_without_umis))
        mc.free()
        m.free()
        c.close()
    return _SEVENTY


def test_seventy_rows_with_an_empty_column():
    """n_rows = 70, rows not contiguous, an empty column, rows with no entry / one entry / no zeros / one distinct value, leading and
    trailing blocks of zeros; every place a trial draw can land and both kinds of first centre occur (asserted on the restatement)"""
    s = _seventy()
    bound = FACTOR * golden()["movement"]
    landings, kinds = np.zeros(4, np.int64), np.zeros(2, np.int64)
    assert not s["dense"][11].any()
    fpc = np.zeros(257, np.int64)
    for p, (counts, cols, ref) in enumerate(s["rows"]):
        got = {k: s["per_feature"][k][p] for k in s["per_feature"]}
        got = dict(fitted=bool(got["status"]), n_iter=int(got["n_iter"]), winner=int(got["winner"]), cells_assigned=int(got["cells_assigned"]),
                   umi_threshold_observed=int(got["umi_threshold_observed"]), weight_low=got["weight_low"], weight_high=got["weight_high"],
                   mean_low=got["mean_low"], mean_high=got["mean_high"], covariance=got["covariance"])
        _same_as_restatement("row %d" % p, got, ref, s["cells"][p].astype(np.int64), cols[ref["calls"]], bound)
        fpc[s["cells"][p]] += 1
        if ref["fitted"]:
            landings += np.bincount(ref["diag"]["landings"], minlength=4)
            kinds += np.bincount(np.array(ref["diag"]["first_is_entry"], int), minlength=2)
    assert landings.min() > 0 and kinds.min() > 0, (landings, kinds)
    assert not s["per_feature"]["status"][0] and s["per_feature"]["status"][1] and int(s["per_feature"]["n_distinct"][1]) == 2      # no entry; one entry
    assert np.array_equal(s["fpc"], fpc) and s["fpc"][11] == 0
    umis = s["dense"][:, s["listed"]].sum(1)
    assert s["tallies"] == (int((fpc == 0).sum()), int((fpc == 1).sum()), int((fpc > 1).sum()), int((umis == 0).sum())) and umis[11] == 0


@pytest.mark.parametrize("n_rows", [1, 3])
def test_a_row_alone_equals_the_row_among_others(n_rows):
    """n_rows = 1 and 3: the same rows fitted alone (or three at a time) are bit-identical to their fit among 70"""
    s = _seventy()
    c, m = _matrix(s["dense"], s["dense"].shape[1])
    for first in ((7,), (3,), (5,)) if n_rows == 1 else ((2, 5, 7), (8, 30, 69)):
        mc = c.marginal_calls(m, s["listed"][list(first)], umi_threshold=3, n_features=s["dense"].shape[1])
        cells = mc.cells_per_feature()
        for q, p in enumerate(first):
            for k in mc.per_feature:
                assert mc.per_feature[k][q].tobytes() == s["per_feature"][k][p].tobytes(), (k, p)
            assert np.array_equal(cells[q], s["cells"][p])
        mc.free()
    m.free()
    c.close()


def _bits(mc):
    out = {k: v.tobytes() for k, v in mc.per_feature.items() if k != "in_lds"}
    indptr, cols = mc.assignments()
    out.update(indptr=indptr.tobytes(), cols=cols.tobytes(), fpc=mc.features_per_cell.tobytes())
    return out


def test_bit_for_bit_between_runs_and_lds_caps(monkeypatch):
    monkeypatch.delenv("CRGPU_MC_LDS_VALUES", raising=False)
    g = golden()
    idx = [i for i in range(len(g["names"])) if int(g["V"][i]) == 5000 and int(g["umi_threshold"][i]) == 1]
    dense, listed = _interleave([fixture_row(i)[4] for i in idx], 9)
    results = {}
    for cap in (None, "0", "8"):      # read when the context is created
        if cap is not None:
            monkeypatch.setenv("CRGPU_MC_LDS_VALUES", cap)
        c, m = _matrix(dense, dense.shape[1])
        a = c.marginal_calls(m, listed, n_features=dense.shape[1])
        b = c.marginal_calls(m, listed, n_features=dense.shape[1])
        assert _bits(a) == _bits(b), cap
        results[cap] = (_bits(a), a.per_feature["in_lds"].copy(), a.per_feature["n_distinct"].copy(), a.per_feature["status"].copy())
        a.free(), b.free(), m.free()
        c.close()
    assert results[None][0] == results["0"][0] == results["8"][0]
    nd, fitted = results[None][2], results[None][3] == 1
    assert nd.max() > 256 and ((nd > 64) & (nd <= 256)).any()                            # one wave and four, more than 64 and more than 256 values
    assert np.array_equal(results[None][1] == 1, fitted & (nd <= 4096)) and not results["0"][1].any()
    assert np.array_equal(results["8"][1] == 1, fitted & (nd <= 8)) and (results["8"][1] == 1).any()


def test_argument_checks_and_moments():
    from cellranger_amd import engine as E

    rng = np.random.RandomState(3)
    V, NF = 90, 40
    dense = rng.poisson(1.0, (V, NF)) * rng.randint(1, 60, (V, NF))
    dense[17] = 0
    c, m = _matrix(dense, NF)
    rows = np.array([1, 4, 9, 30], np.uint32)
    for bad_rows, thr in ((rows, 0), (rows[::-1].copy(), 1), (np.array([2, 2], np.uint32), 1), (np.array([2, NF], np.uint32), 1)):
        with pytest.raises(E.CrgpuError) as ei:
            c.marginal_calls(m, bad_rows, umi_threshold=thr, n_features=NF)
        assert ei.value.code == EINVAL
    sx, sxx, sxy = c.tag_moments(m, rows, NF)
    sub = dense[:, rows].astype(np.int64)
    assert np.array_equal(sx, sub.sum(0)) and np.array_equal(sxx, (sub * sub).sum(0)) and np.array_equal(sxy, sub.T @ sub)
    with pytest.raises(E.CrgpuError) as ei:
        c.tag_moments(m, np.arange(17, dtype=np.uint32), NF)
    assert ei.value.code == ERANGE
    m.free()
    c.close()


def test_protospacers_and_antibodies():
    from cellranger_amd import engine as E

    V = 257
    rows = _synthetic_rows(V, 12, 3)
    dense, listed = _interleave([r[0] for r in rows], 13)
    c, m = _matrix(dense, dense.shape[1])
    got = E.call_protospacers(c, m, listed, n_features=dense.shape[1])
    fpc = np.zeros(V, np.int64)
    for counts, cols, ref in rows:
        fpc[cols[ref["calls"]]] += 1
    n1, nm = int((fpc == 1).sum()), int((fpc > 1).sum())
    assert np.array_equal(got["calls"].features_per_cell, fpc)
    assert got["metrics"] == {"CRISPR_frac_cells_with_protospacer": n1 / V + nm / V, "CRISPR_frac_cells_with_single_protospacer": n1 / V,
                              "CRISPR_frac_cells_with_multiple_protospacer": nm / V}
    assert got["summary"]["1 protospacer assigned"][0] == n1 and got["summary"]["More than 1 protospacer assigned"][0] == nm
    assert got["summary"]["No confident call"][0] == V - n1 - nm
    assert got["summary"]["No guide molecules"][0] == int((dense[:, listed].sum(1) == 0).sum())
    assert got["umi_thresholds"] == {p: r[2]["umi_threshold_observed"] for p, r in enumerate(rows) if r[2]["cells_assigned"]}
    got["calls"].free()
    # antibodies: only CD3 / CD19 / CD14, and of those only a feature with at least 1000 UMIs, are called (threshold 1)
    ids = [b"CD3", b"CD4", b"CD19", b"CD8", b"AB0", b"CD14"] + [b"AB%d" % i for i in range(1, 7)]
    tot = dense[:, listed].sum(0)
    assert tot[0] < 1000 <= tot[2] and tot[5] >= 1000      # CD3 is the row without an entry
    ab = E.call_antibodies(c, m, listed, ids, n_features=dense.shape[1])
    assert ab["called_ids"] == [b"CD19", b"CD14"] and list(ab["called_rows"]) == [listed[2], listed[5]]
    fpc = np.zeros(V, np.int64)
    for p in (2, 5):
        counts = dense[:, listed[p]]
        cols = np.flatnonzero(counts)
        fpc[cols[R.fit_histogram(V, cols, counts[cols], 1)["calls"]]] += 1
    assert np.array_equal(ab["calls"].features_per_cell, fpc)
    assert ab["metadata"]["num_singlets"] == int((fpc == 1).sum()) and ab["metadata"]["num_multiplets"] == int((fpc > 1).sum())
    assert ab["metadata"]["num_cells_without_feature_umis"] == int((dense[:, listed].sum(1) == 0).sum())
    ab["calls"].free()
    m.free()
    c.close()


def test_marginal_to_jibes_chain():
    """a small synthetic CMO well: filtered matrix -> call_tags_marginal -> call_tags_jibes, against the same chain through the two
    restatements (marginal_calls_numpy, jibes_numpy); no scikit-learn in the path"""
    from cellranger_amd import engine as E

    rng = np.random.RandomState(41)
    V, k = 400, 5
    owner = rng.randint(0, 4, V)
    tags = rng.poisson(3.0, (V, k)).astype(np.int64)
    for t in range(4):
        tags[owner == t, t] += rng.poisson(250, int((owner == t).sum()))
    doublets = rng.choice(V, 30, replace=False)
    tags[doublets, (owner[doublets] + 1) % 4] += rng.poisson(250, 30)
    tags[:, 4] = rng.poisson(0.4, V)                          # a tag of fewer than 1000 UMIs: a contaminant
    tags[rng.choice(V, 12, replace=False)] = 0                # near-zero barcodes
    ids = [b"CMO303", b"CMO301", b"CMO304", b"CMO302", b"CMO300"]
    dense, listed = _interleave([tags[:, t] for t in range(k)], 17)
    c, m = _matrix(dense, dense.shape[1])
    mar = E.call_tags_marginal(c, m, listed, ids, n_features=dense.shape[1])
    # the restatement of the marginal stage
    order = np.argsort(np.array(ids))
    flags, src = R.identify_contaminants(tags.T, order)
    fits = []
    for t in range(k):
        cols = np.flatnonzero(tags[:, t])
        fits.append((cols, R.fit_histogram(V, cols, tags[cols, t], 1)))
    assert np.array_equal(mar["flags"], flags) and list(flags) == [0, 0, 0, 0, 1]
    assert mar["source_tags"] == [[ids[j] for j in s] for s in src]
    fpc = np.zeros(V, np.int64)
    called = []
    for t, (cols, f) in enumerate(fits):
        called.append(cols[f["calls"]])
        assert np.array_equal(mar["calls"].cells_per_feature()[t], called[t])
        if flags[t] == 0:
            fpc[called[t]] += 1
        want_snr = R.umi_interval_snr(tags[:, t], f["umi_threshold_observed"]) if len(called[t]) else np.nan
        assert mar["log10_snr"][t] == want_snr or (np.isnan(want_snr) and np.isnan(mar["log10_snr"][t])), t
    assert np.array_equal(mar["features_per_cell"], fpc) and np.array_equal(mar["nlet_observed"], np.bincount(fpc, minlength=15)[:15])
    valid = np.array([flags[t] == 0 and len(called[t]) > 0 for t in range(k)])
    place = np.cumsum(valid) - 1
    prelim = np.full(V, -1, np.int32)
    for t in np.flatnonzero(valid):
        one = called[t][fpc[called[t]] == 1]
        prelim[one] = place[t]
    assert np.array_equal(mar["valid_tags"], valid) and np.array_equal(mar["prelim_calls"], prelim) and valid.sum() == 4 and (prelim >= 0).sum() > 200
    # JIBES on top, both ways
    _, _, kept, _ = JR.tag_table(tags, valid)
    est = JR.expected_total_cells(len(kept), 2000)
    got = E.call_tags_jibes(c, m, listed, mar["valid_tags"], mar["prelim_calls"], n_gems=2000, n_features=dense.shape[1], estimated_cells=est,
                            tag_names=ids, confidence=0.5)
    ref = JR.call_tags(tags, valid, prelim, 2000, confidence=0.5, estimated_cells=est)
    assert got["fit"]["iterations"] == ref["fit"]["iterations"] and got["fit"]["converged"]
    names = [i.decode() for i, v in zip(ids, valid) if v]
    for t, nm in enumerate(names):
        assert got["barcodes_per_tag"][nm] == ref["per_tag"][t], nm
    assert got["non_singlets"] == ref["non_singlets"] and sum(len(v) for v in got["barcodes_per_tag"].values()) > 200
    mar["calls"].free()
    m.free()
    c.close()
