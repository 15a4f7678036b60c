"""GPU tests of the EmptyDrops step (Context.call_additional_cells -> crgpu_emptydrops_dev, crgpu_ambient_pvalues_dev and the
simulation kernel on its own).

The expected values come from tests/emptydrops_numpy.py, which tests/test_emptydrops_restatement.py pins against the reference's
recorded outputs.  Integers (ambient set size, thresholds, candidates, totals, eval_features, distinct N, called columns, the
filtered CSC) are compared for equality; profile_p and the observed log-likelihoods at the relative RTOL of that file; the
simulated table at `1e-12 relative + N * 2^-40`: the device sums 2 N log terms rounded to 2^-40 each (at most 2^-41 off), the
restatement sums the f64 terms in extended precision.  n_lower (simulated values strictly below the observed one) is an integer
made from two floating values: it must lie between the number of restated values below the observed one by more than 1e-9
(relative) and that number plus the restated values within 1e-9 of it -- equality wherever no value is that close, which the
fixtures with recorded tables assert outright."""
import numpy as np
import pytest

import emptydrops_numpy as R
from test_emptydrops_restatement import RTOL, load_fixture

pytestmark = pytest.mark.gpu
N_1M = 1_000_000
WL = 8192


# ---- helpers ------------------------------------------------------------------------------------------------------------------
def _ctx():
    import gpu_helpers as G

    c = G.fresh_ctx()
    c.set_whitelist(0, np.arange(WL, dtype=np.uint32), length=16)      # rank == value: column k is barcode k
    return c


def _matrix(c, indptr, indices, data):
    """MatrixDev of a CSC whose column k is the k-th whitelist entry"""
    V = len(indptr) - 1
    seen = np.zeros(c.n_canon, np.uint32)
    seen[:V] = 1
    c.set_counts(0, 0, seen)
    bc = np.repeat(np.arange(V, dtype=np.uint32), np.diff(indptr))
    m = c.assemble_matrix_dev(c.upload(bc), c.upload(indices.astype(np.uint32)), c.upload(data.astype(np.uint32)), len(indices))
    assert m.n_barcodes == V and m.nnz == len(indices)
    return m


def _initial(c, m, cells):
    from cellranger_amd import engine as E

    cells = np.ascontiguousarray(cells, dtype=np.uint64)
    return E.CellCall(c, c.upload(cells) if len(cells) else c.empty(0, np.uint64), len(cells), {"filtered_bcs": len(cells)}, m)


def _close(a, b, rtol=RTOL):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool(np.all(np.abs(a - b) <= rtol * np.abs(b)))


def _table_close(tab, ref, sim_n):
    bound = 1e-12 * np.abs(ref) + np.asarray(sim_n, np.float64)[:, None] * 2.0 ** -40
    print("table: largest |dev - ref| / bound = %.3g" % np.max(np.abs(tab - ref) / bound))
    return tab.shape == ref.shape and bool(np.all(np.abs(tab - ref) <= bound))


def _n_lower_ok(n_lower, obs, umis, sim_n, ref_table, need_exact=False):
    rows = ref_table[np.searchsorted(sim_n, umis)]
    tol = 1e-9 * np.abs(obs)[:, None]
    sure = np.sum(rows < obs[:, None] - tol, axis=1)
    maybe = np.sum(np.abs(rows - obs[:, None]) <= tol, axis=1)
    if need_exact:
        assert not maybe.any()
    return bool(np.all((sure <= n_lower) & (n_lower <= sure + maybe)))


def _csc_select(indptr, indices, data, cols):
    lens = np.diff(indptr)[cols]
    take = np.concatenate([np.arange(indptr[c], indptr[c + 1]) for c in cols] + [np.zeros(0, np.int64)]).astype(np.int64)
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), indices[take], data[take]


def _check_integers(a, ref):
    m = a.metrics
    assert a.status == ref["status"] == m["status"]
    assert m["n_ambient_used"] == ref["n_ambient_used"] and m["max_background_umis"] == ref["max_background_umis"]
    assert m["emptydrops_minimum_umis"] == ref["emptydrops_minimum_umis"]
    if ref["status"] != R.STATUS_OK:
        assert m["n_nonambient"] == 0 and len(a.eval_cols) == 0 and len(a.is_nonambient) == 0
        return
    assert np.array_equal(a.eval_cols, ref["eval_cols"]) and np.array_equal(a.umis, ref["umis"])
    assert m["n_candidates"] == len(ref["eval_cols"]) and m["n_distinct_n"] == len(np.unique(ref["umis"]))
    assert m["n_eval_features"] == len(ref["eval_features"]) and np.array_equal(a.eval_features, ref["eval_features"])


def _check_floats(a, ref):
    assert _close(a.profile_p, ref["profile_p"]) and abs(a.profile_p.sum() - 1) < 1e-12
    assert _close([a.metrics["sgt_p0"], a.metrics["sgt_slope"]], [ref["sgt_p0"], ref["sgt_slope"]])
    assert _close(a.obs_loglk, ref["obs_loglk"])


def _check_calls(a, ref, cells, need_exact=False):
    """p-values, BH and calls follow from n_lower exactly as in the restatement; n_lower within its rounding bound"""
    S = ref["sim_loglk"].shape[1]
    assert _n_lower_ok(a.n_lower, a.obs_loglk, a.umis, ref["sim_n"], ref["sim_loglk"], need_exact)
    assert np.array_equal(a.pvalues, (1 + a.n_lower.astype(np.int64)).astype(float) / (1 + S))
    assert np.array_equal(a.pvalues_adj, R.adjust_pvalue_bh(a.pvalues))
    assert np.array_equal(a.is_nonambient, a.pvalues_adj <= 0.01) and a.metrics["n_nonambient"] == a.is_nonambient.sum()
    want = np.union1d(np.asarray(cells, np.int64), a.eval_cols[a.is_nonambient].astype(np.int64))
    assert a.call.n_cells == len(want) and np.array_equal(a.call.cols_host(), want.astype(np.uint64))


def _tie_well(seed):
    """ambient totals of 1 - 99 over 1500 droplets: every total occurs ~15 times, so both ends of the range cut a plateau"""
    return R.make_well(seed, n_features=300, n_cells=40, n_ambient=1500, n_big_ambient=30, n_small_cells=20)


# ---- 5 / 6: integers, profile and observed log-likelihood, with and without a mask, on cut plateaus -------------------------------
@pytest.mark.parametrize("masked", [False, True], ids=["all_features", "masked"])
def test_ambient_set_candidates_profile_and_observed_loglk(masked):
    indptr, indices, data, nf, kind = _tie_well(21)
    mask = None
    if masked:
        mask = np.ones(nf, np.uint8)
        mask[: nf // 3] = 0
    low, high = 300, 900
    umis = R.column_sums(indptr, indices, data, nf, mask)
    desc = np.sort(umis)[::-1]
    assert desc[low - 1] == desc[low] and desc[high - 1] == desc[high] and desc[high] > 0       # both cuts fall inside a plateau
    cells = np.flatnonzero(kind == 0)
    ref = R.find_nonambient(indptr, indices, data, nf, cells, low, high, 50, 100, 0.01, 0, mask)
    assert ref["status"] == R.STATUS_OK and len(ref["eval_cols"]) > 30
    # the tie rule matters here: the other order of equal totals gives another profile
    other = np.argsort(umis[::-1], kind="stable")[low:high]
    other = np.sort(len(umis) - 1 - other)
    assert not np.array_equal(np.sort(other[umis[other] > 0]), R.ambient_set(umis, low, high)[0])
    c = _ctx()
    m = _matrix(c, indptr, indices, data)
    a = c.call_additional_cells(m, _initial(c, m, cells), low, high, emptydrops_minimum_umis=50, num_sims=100, feature_mask=mask,
                                keep_sim_table=True)
    _check_integers(a, ref)
    _check_floats(a, ref)
    assert np.array_equal(a.sim_n, ref["sim_n"]) and _table_close(a.sim_loglk, ref["sim_loglk"], ref["sim_n"])
    _check_calls(a, ref, cells)
    c.close()


# ---- 7: a supplied table: the reference's p-values, BH and calls bit for bit -------------------------------------------------------
def test_supplied_reference_table_gives_the_references_pvalues():
    g, (indptr, indices, data, nf), kind, cells = load_fixture()
    tc, fdr = g["tab_cand"], float(g["fdr"])
    umis, obs = g["umis"][tc], g["ref_obs_loglk"][tc]
    assert not R.near_tie(obs, umis, g["tab_n"], g["tab_loglk"])
    c = _ctx()
    n_lower, p, q, call = c.ambient_pvalues(umis, obs, g["tab_n"], g["tab_loglk"], fdr)
    assert np.array_equal(p, g["tab_pvalues"]) and np.array_equal(q, g["tab_pvalues_adj"]) and np.array_equal(call, g["tab_pvalues_adj"] <= fdr)
    assert np.array_equal(n_lower, R.count_lower(umis, obs, g["tab_n"], g["tab_loglk"]))
    # ... and through the whole step: every other candidate joins the initial cells, the device's own observed values are compared
    others = np.setdiff1d(g["eval_cols"], g["eval_cols"][tc])
    init = np.union1d(cells, others)
    m = _matrix(c, indptr, indices, data)
    S = g["tab_loglk"].shape[1]
    a = c.call_additional_cells(m, _initial(c, m, init), int(g["low"]), int(g["high"]), int(g["minimum_umis"]), num_sims=S, max_adj_pvalue=fdr,
                                sim_table=(g["tab_n"], g["tab_loglk"]))
    assert a.status == 0 and np.array_equal(a.eval_cols, g["eval_cols"][tc]) and np.array_equal(a.umis, umis)
    assert _close(a.obs_loglk, obs) and not R.near_tie(a.obs_loglk, umis, g["tab_n"], g["tab_loglk"])
    assert np.array_equal(a.pvalues, g["tab_pvalues"]) and np.array_equal(a.pvalues_adj, g["tab_pvalues_adj"])
    assert np.array_equal(a.is_nonambient, g["tab_pvalues_adj"] <= fdr)
    assert np.array_equal(a.call.cols_host(), np.union1d(init, a.eval_cols[a.is_nonambient].astype(np.int64)).astype(np.uint64))
    # a total without a row is refused
    from cellranger_amd import engine as E

    with pytest.raises(E.CrgpuError) as ei:
        c.ambient_pvalues(np.array([int(g["tab_n"][0]) + 100000]), obs[:1], g["tab_n"], g["tab_loglk"], fdr)
    assert ei.value.code == -1
    c.close()


# ---- 8: the simulation kernel against the restatement ----------------------------------------------------------------------------
def _lognormal_profile(seed, n):
    rs = np.random.RandomState(seed)
    p = np.exp(rs.normal(0, 2, n))
    return p / p.sum()


def _half_profile():
    p = _lognormal_profile(5, 200) * 0.5
    p[17] += 0.5
    return p / p.sum()


SIM_CASES = {
    "single_n": (_lognormal_profile(1, 300), [37, 37, 37], 64),
    "steps_of_one_more_sims_than_workgroups": (_lognormal_profile(2, 50), list(range(5, 41)), 1100),
    "step_longer_than_a_workgroup_pass": (_lognormal_profile(3, 2000), [10, 9010, 9013], 48),   # a pass = 1024 threads x 4 draws
    "one_feature_at_half": (_half_profile(), [64, 3000, 3001], 64),
    "one_feature": (np.array([1.0]), [1, 5, 700], 16),
    "two_features": (np.array([0.3, 0.7]), [1, 2, 3, 50, 4100], 64),
    "guide_bucket_edges": (np.array([0.25, 0.25, 2.0 ** -30, 0.5 - 2.0 ** -30]), [500, 501], 64),
}


def _observed_between(ref_table, sim_n, umis, q=0.4):
    """an observed value per candidate from the RESTATED row of its N: half way between two neighbouring simulated values, or
    1 below when those two are (nearly) the same value"""
    rows = np.sort(ref_table[np.searchsorted(sim_n, umis)], axis=1)
    k = int(q * (rows.shape[1] - 1))
    mid = 0.5 * (rows[:, k] + rows[:, k + 1])
    return np.where(rows[:, k + 1] - rows[:, k] <= 1e-6, rows[:, k] - 1.0, mid)


@pytest.mark.parametrize("case", sorted(SIM_CASES))
def test_simulation_equals_the_restatement(case, monkeypatch):
    p, umis, S = SIM_CASES[case]
    umis = np.array(umis)
    sim_n, ref = R.simulate_philox(p, umis, S, seed=3)
    obs = _observed_between(ref, sim_n, umis)
    monkeypatch.delenv("CRGPU_ED_LDS_FEATURES", raising=False)
    c = _ctx()
    n, tab, n_lower, _ = c.emptydrops_simulate(p, umis, S, seed=3, obs_loglk=obs)
    assert np.array_equal(n, sim_n) and _table_close(tab, ref, sim_n)
    assert _n_lower_ok(n_lower, obs, umis, sim_n, ref)
    assert np.array_equal(n_lower, np.sum(tab[np.searchsorted(sim_n, umis)] < obs[:, None], axis=1))     # counters == the kept table
    # the same call twice; another seed
    n2, tab2, n_lower2, _ = c.emptydrops_simulate(p, umis, S, seed=3, obs_loglk=obs)
    assert np.array_equal(tab, tab2) and np.array_equal(n_lower, n_lower2)
    if len(p) > 1:
        assert not np.array_equal(c.emptydrops_simulate(p, umis, S, seed=4)[1], tab)
    c.close()
    # counters in global memory: bit-identical
    monkeypatch.setenv("CRGPU_ED_LDS_FEATURES", "0")       # read when the context is created
    cg = _ctx()
    n3, tab3, n_lower3, _ = cg.emptydrops_simulate(p, umis, S, seed=3, obs_loglk=obs)
    assert np.array_equal(n3, sim_n) and np.array_equal(tab3, tab) and np.array_equal(n_lower3, n_lower)
    cg.close()


# ---- 9: the planted well -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planted():
    g, csc, kind, _ = load_fixture()
    cells = np.flatnonzero(kind == 0)
    S = int(g["num_sims"])
    ref = R.find_nonambient(*csc, cells, int(g["low"]), int(g["high"]), int(g["minimum_umis"]), S, float(g["fdr"]), seed=0)
    return g, csc, kind, cells, S, ref


def test_planted_well(planted, monkeypatch):
    g, (indptr, indices, data, nf), kind, cells, S, ref = planted
    out = []
    for lds in (None, "0"):
        if lds is None:
            monkeypatch.delenv("CRGPU_ED_LDS_FEATURES", raising=False)
        else:
            monkeypatch.setenv("CRGPU_ED_LDS_FEATURES", lds)
        c = _ctx()
        m = _matrix(c, indptr, indices, data)
        a = c.call_additional_cells(m, _initial(c, m, cells), int(g["low"]), int(g["high"]), int(g["minimum_umis"]), num_sims=S,
                                    max_adj_pvalue=float(g["fdr"]), seed=0)
        assert a.metrics["sim_in_lds"] == (lds is None) and a.sim_loglk is None
        _check_integers(a, ref)
        _check_floats(a, ref)
        _check_calls(a, ref, cells)
        k = kind[a.eval_cols.astype(np.int64)]
        assert (k == 3).sum() == 60 and a.is_nonambient[k == 3].all() and np.all(a.pvalues[k == 3] == 1.0 / (S + 1))
        assert np.array_equal(a.is_nonambient, ref["is_nonambient"])                  # the calls equal the restatement's everywhere
        assert np.array_equal(a.call.cols_host(), ref["called_cols"].astype(np.uint64))
        cols = ref["called_cols"]
        rank, f_indptr, f_indices, f_data = a.call.filtered_matrix().download()
        e_indptr, e_indices, e_data = _csc_select(indptr, indices, data, cols)
        assert np.array_equal(rank, cols.astype(np.uint32)) and np.array_equal(a.call.ranks, cols.astype(np.uint32))
        assert np.array_equal(f_indptr, e_indptr) and np.array_equal(f_indices, e_indices) and np.array_equal(f_data, e_data)
        out.append((a.n_lower, a.obs_loglk, a.pvalues_adj))
        c.close()
    for x, y in zip(*out):
        assert np.array_equal(x, y)                                                   # LDS and global counters: bit-identical


# ---- 10: the four ways out without additional cells ------------------------------------------------------------------------------
@pytest.mark.parametrize("status", [R.STATUS_NO_AMBIENT, R.STATUS_SGT, R.STATUS_NO_CELLS, R.STATUS_NO_CANDIDATES])
def test_status_paths_keep_the_initial_call(status):
    kw = dict(low=300, high=900, emptydrops_minimum_umis=50)
    if status == R.STATUS_SGT:
        indptr, indices, data, nf, kind = R.make_well(4, n_features=8, n_cells=40, n_ambient=1500, n_big_ambient=30, n_small_cells=20)
    else:
        indptr, indices, data, nf, kind = _tie_well(22)
    cells = np.flatnonzero(kind == 0)
    if status == R.STATUS_NO_AMBIENT:
        kw.update(low=len(kind) + 5, high=len(kind) + 500)
    elif status == R.STATUS_NO_CELLS:
        cells = cells[:0]
    elif status == R.STATUS_NO_CANDIDATES:
        kw.update(emptydrops_minimum_umis=10 ** 7)
    ref = R.find_nonambient(indptr, indices, data, nf, cells, kw["low"], kw["high"], kw["emptydrops_minimum_umis"], 50)
    assert ref["status"] == status
    c = _ctx()
    m = _matrix(c, indptr, indices, data)
    a = c.call_additional_cells(m, _initial(c, m, cells), num_sims=50, **kw)
    assert a.status == status and a.status_text
    _check_integers(a, ref)
    assert a.call.n_cells == len(cells) and np.array_equal(a.call.cols_host(), cells.astype(np.uint64))
    assert np.array_equal(a.call.ranks, cells.astype(np.uint32))
    f = a.call.filtered_matrix()
    e_indptr, e_indices, e_data = _csc_select(indptr, indices, data, cells)
    _, f_indptr, f_indices, f_data = f.download()
    assert np.array_equal(f_indptr, e_indptr) and np.array_equal(f_indices, e_indices) and np.array_equal(f_data, e_data)
    c.close()


def test_bad_arguments_are_refused():
    from cellranger_amd import engine as E

    indptr, indices, data, nf, kind = _tie_well(22)
    cells = np.flatnonzero(kind == 0)
    c = _ctx()
    m = _matrix(c, indptr, indices, data)
    for bad_cells in (cells[::-1], np.append(cells, len(kind))):       # not ascending; out of range
        with pytest.raises(E.CrgpuError) as ei:
            c.call_additional_cells(m, _initial(c, m, bad_cells), 300, 900, 50, num_sims=10)
        assert ei.value.code == -1
    with pytest.raises(E.CrgpuError) as ei:
        c.call_additional_cells(m, _initial(c, m, cells), 300, 900, 50, num_sims=10, feature_mask=np.ones(nf // 2, np.uint8))
    assert ei.value.code == -1
    a = c.call_additional_cells(m, _initial(c, m, cells), 300, 900, 50, num_sims=10)     # the context is still usable
    assert a.status == 0
    c.close()


# ---- 11: end to end ------------------------------------------------------------------------------------------------------------
def test_end_to_end_from_reads_to_the_filtered_matrix():
    """the 1 M-read workload of the cell-calling test through pass A / B and the count stage -> raw MatrixDev -> the initial call ->
    the additional cells (all features, and with a feature range masked out) -> the filtered matrix"""
    import gpu_helpers as G
    from cellranger_amd import synth as S

    w = S.Workload(n_total=N_1M, seed=S.SEED0 + 3, n_cells=300, n_ambient=20000)
    r = w.host_reads(0, N_1M)
    c = G.fresh_ctx()
    c.set_whitelist(0, w.wl_packed, length=16)
    _, _, _, dev = G.gpu_barcode_stage(c, r, N_1M)
    c.set_key_layout(w.n_genes, w.umi_len, 1, 0)
    counts = c.count_records(c.records(N_1M, w.umi_len, dev["idx"], c.upload(r["umi"]), c.upload(r["umi_qualn"]), c.upload(r["feature"]),
                                       dev["flags"]))
    raw = c.assemble_matrix_dev(*counts.triplets_dev(), counts.n_triplets)
    rank, indptr, indices, data = raw.download()
    V = raw.n_barcodes
    assert V > 10_000
    low, high = V // 40, V // 4            # scaled to the well: the cells are the top ~1 % of its columns
    for mask in (None, np.concatenate([np.ones(w.n_genes // 2, np.uint8), np.zeros(w.n_genes - w.n_genes // 2, np.uint8)])):
        call = c.call_cells_ordmag(c.column_sums(raw, mask), recovered_cells=250)
        call._matrix = raw
        cells = call.cols_host().astype(np.int64)
        ref = R.find_nonambient(indptr, indices, data, w.n_genes, cells, low, high, 5, 200, 0.01, 0, mask)
        assert ref["status"] == R.STATUS_OK and len(ref["eval_cols"]) > 100
        a = c.call_additional_cells(raw, call, low, high, emptydrops_minimum_umis=5, num_sims=200, feature_mask=mask, keep_sim_table=True)
        _check_integers(a, ref)
        _check_floats(a, ref)
        assert np.array_equal(a.sim_n, ref["sim_n"]) and _table_close(a.sim_loglk, ref["sim_loglk"], ref["sim_n"])
        _check_calls(a, ref, cells)
        cols = a.call.cols_host().astype(np.int64)
        f_rank, f_indptr, f_indices, f_data = a.call.filtered_matrix().download()
        e_indptr, e_indices, e_data = _csc_select(indptr, indices, data, cols)
        assert np.array_equal(f_rank, rank[cols]) and np.array_equal(a.call.ranks, rank[cols])
        assert np.array_equal(f_indptr, e_indptr) and np.array_equal(f_indices, e_indices) and np.array_equal(f_data, e_data)
    c.close()
