"""The aggregate stage on the device (Context.remove_aggregates and the entries behind it, Counts.corrected_reads_per_column) against
the restatement tests/aggregates_numpy.py under its tie rule "high", which tests/test_aggregates_restatement.py pins against the
reference's recorded outputs.  Everything is compared for equality, floats as bit patterns.  Contexts and matrices come from
tests/aggregates_gpu.py.  CRGPU_AGG_LDS_ROWS is read when a context is
created: unset (one slice of the LDS when the table fits it, else device memory), 3 (several slices, the last one partial), 0 (the
table in device memory)."""
import numpy as np
import pytest

import aggregates_numpy as R
from aggregates_gpu import ctx as _ctx, matrix as _matrix

pytestmark = pytest.mark.gpu
EINVAL, ESTATE, ERANGE = -1, -5, -6
LDS = (None, "3", "0")
_shared = {}


def _ref(name, fx):
    if ("ref", name) not in _shared:
        _shared[("ref", name)] = R.remove_aggregates(fx, "high")
    return _shared[("ref", name)]


def _bits(x):
    return np.float64(x).view(np.uint64)


def _same(c, m, fx, ref, lds=None, check_matrix=False):
    """Context.remove_aggregates of a fixture against the restatement's dict"""
    from cellranger_amd import engine as E

    clean, agg = c.remove_aggregates(m, fx["kind"], fx.get("num_probe_barcodes"), reads=fx.get("reads"), corrected_reads=fx.get("corrected"))
    assert np.array_equal(agg.removed_cols, ref["removed"]), (agg.removed_cols, ref["removed"])
    assert np.array_equal(agg.reasons, ref["reasons"])
    assert agg.n_kept == len(ref["kept"]) and np.array_equal(agg.kept.to_host(agg.n_kept), ref["kept"])
    if ref["info"] is None:
        assert agg.info is None
    else:
        for k, v in ref["info"].items():
            assert agg.info[k] == v, (k, agg.info[k], v)
        assert agg.info["n_aggregates"] == int((ref["reasons"] & R.COUNTS != 0).sum())
        if ref["info"]["n_candidates"]:      # the rank pass ran
            n_signal = ref["info"]["n_signal"]
            if lds == "0":
                assert (agg.info["in_lds"], agg.info["rows_per_slice"], agg.info["n_slices"]) == (0, 0, 1)
            elif lds is not None:      # slices of at most that many rows, and of what the 160 KB of LDS hold
                Kc = ref["info"]["n_candidates"]
                rows = min(int(lds), (160 * 1024 - 64) // (8 * Kc + 4 * (Kc + 1)), n_signal)
                assert (agg.info["in_lds"], agg.info["rows_per_slice"], agg.info["n_slices"]) == (1, rows, -(-n_signal // rows))
            else:
                assert agg.info["in_lds"] == 1 and agg.info["n_slices"] * agg.info["rows_per_slice"] >= n_signal
    if ref["antigen_threshold"] is None:
        assert agg.antigen_threshold is None
    else:
        assert _bits(agg.antigen_threshold) == _bits(ref["antigen_threshold"])
    assert sorted(agg.libraries) == sorted(ref["libraries"])
    for lib, exp in ref["libraries"].items():
        got = agg.libraries[lib]
        for k in ("number_aggregate_GEMs", "reads_removed", "reads_total"):
            assert got[k] == exp[k], (lib, k, got[k], exp[k])
        for k in ("cols", "umis", "reads", "corrected_reads"):
            assert (k in got) == (k in exp) and (k not in exp or np.array_equal(got[k], exp[k])), (lib, k)
        if "reads" in exp:
            assert np.array_equal(got["frac_total_reads"], exp["reads"] / np.float64(exp["reads_total"]))
        if "corrected_reads" in exp:
            assert np.array_equal(got["frac_corrected_reads"], exp["corrected_reads"] / exp["reads"].astype(np.float64))
    metrics = E.aggregate_metrics(agg)
    for lib, exp in ref["libraries"].items():
        prefix = {R.AB: "ANTIBODY_", R.AG: "ANTIGEN_"}[lib]
        assert metrics[prefix + "number_aggregate_GEMs"] == exp["number_aggregate_GEMs"]
        lost = metrics[prefix + "reads_lost_to_aggregate_GEMs"]
        assert lost is None if exp["reads_total"] is None else _bits(lost) == _bits(exp["reads_removed"] / exp["reads_total"])
    if check_matrix:
        rank, indptr, indices, data = clean.download()
        e_ptr, e_idx, e_data = R.select_barcodes(fx["indptr"], fx["indices"], fx["data"], ref["kept"])
        assert np.array_equal(rank, ref["kept"].astype(np.uint32)) and np.array_equal(indptr, e_ptr)
        assert np.array_equal(indices, e_idx) and np.array_equal(data, e_data)
    clean.free()
    return agg


# ---- the recorded fixtures in every form of the rank pass --------------------------------------------------------------------------
@pytest.mark.parametrize("lds", LDS)
@pytest.mark.parametrize("name", [n for n, _ in R.golden_fixtures()])
def test_golden_fixtures_in_every_form(name, lds):
    fx = dict(R.golden_fixtures())[name]
    c = _ctx(lds)
    m = _matrix(c, fx)
    _same(c, m, fx, _ref(name, fx), lds, check_matrix=lds is None)
    m.free()


# ---- fixtures that tell the failure modes apart --------------------------------------------------------------------------------------
def _kinds(n_gex, n_ab, n_ag=0):
    return np.array([R.KIND_OTHER] * n_gex + [R.KIND_ANTIBODY] * n_ab + [R.KIND_ANTIGEN] * n_ag, np.uint8)


@pytest.mark.parametrize("lds", LDS)
@pytest.mark.parametrize("npb", [None, 2])
def test_constant_matrix_every_value_ties(npb, lds):
    """every count is 50: the candidates and the top K of every row are decided by the column alone, the K highest columns"""
    K, V = 25 * (npb or 1), 120
    fx = R.from_dense(np.full((8, V), 50), _kinds(2, 6), num_probe_barcodes=npb)
    ref = R.remove_aggregates(fx, "high")
    assert list(ref["removed"]) == list(range(V - K, V)) and list(R.remove_aggregates(fx, "low")["removed"]) == list(range(K))
    c = _ctx(lds)
    m = _matrix(c, fx)
    _same(c, m, fx, ref, lds)
    m.free()


def _sparse_row_fixture():
    """6 signal antibodies, all of them needed (int(round(6 * 0.98)) == 6).  Rows 2 .. 6 are dense; row 7 has 9 non-zero entries (fewer
    than K = 25), in columns 0 .. 9 without 3.  Five planted columns are high in the dense rows and ZERO in row 7: there they rank
    among the implicit zeros, by column.  The top 25 of row 7 are its 9 entries and the 16 zeros of the highest columns, 64 .. 79: the
    planted columns 70, 75 and 78 pass, 3 and 40 do not."""
    rng = np.random.RandomState(3)
    V = 80
    dense = np.zeros((8, V), np.int64)
    dense[:2] = rng.poisson(1.0, (2, V))
    dense[2:7] = rng.poisson(30, (5, V))
    for c in (3, 40, 70, 75, 78):
        dense[2:7, c] = 1000 + c
    dense[7, [0, 1, 2, 4, 5, 6, 7, 8, 9]] = 200
    return R.from_dense(dense, _kinds(2, 6))


@pytest.mark.parametrize("lds", LDS)
def test_a_candidate_that_is_zero_in_a_row_of_fewer_than_k_entries(lds):
    fx = _sparse_row_fixture()
    ref = R.remove_aggregates(fx, "high")
    assert ref["info"]["n_signal"] == 6 and ref["info"]["min_antibodies"] == 6
    assert list(ref["removed"]) == [70, 75, 78]
    c = _ctx(lds)
    m = _matrix(c, fx)
    _same(c, m, fx, ref, lds)
    m.free()


def _beyond_fixture():
    """V = 30, K = 25, 6 signal antibodies, all needed.  Rows 1 .. 5 are dense and low in columns 10 .. 14, which are therefore no
    candidates and outside every dense row's top 25.  Row 6 has 10 entries, in columns 20 .. 29.  A candidate c < 20 is ZERO there: above
    it are the 10 entries and the zeros of a higher column, (29 - c) - 10 of them, since the 10 columns beyond it that hold an entry
    are no zeros: 29 - c pairs, fewer than 25 for c >= 5.  Counting all 29 - c higher columns as zeros gives 39 - c and passes only c >= 15:
    columns 5 .. 9 are decided by the subtracted term."""
    dense = np.zeros((7, 30), np.int64)
    for r in range(1, 6):
        dense[r] = 100 + 3 * r + np.arange(30)
        dense[r, 10:15] = 40 + np.arange(5)
    dense[6, 20:] = 200
    return R.from_dense(dense, _kinds(1, 6))


@pytest.mark.parametrize("lds", LDS)
def test_entries_beyond_a_zero_candidate_are_not_counted_as_zeros(lds):
    fx = _beyond_fixture()
    ref = R.remove_aggregates(fx, "high")
    assert ref["info"]["n_signal"] == 6 and ref["info"]["min_antibodies"] == 6 and ref["info"]["n_candidates"] == 25
    assert list(ref["removed"]) == list(range(5, 10)) + list(range(15, 30))
    c = _ctx(lds)
    m = _matrix(c, fx)
    _same(c, m, fx, ref, lds)
    m.free()


@pytest.mark.parametrize("V", [7, 25, 26, 100, 101])
def test_fewer_columns_than_k_and_the_antigen_top_100(V):
    """V < K and V == K: every column is a candidate and among the top K of every row.  The antigen step takes min(100, V) columns: with
    V = 101 the lowest column falls out of the top, with V <= 100 the quantiles run over all of them"""
    rng = np.random.RandomState(V)
    dense = np.zeros((9, V), np.int64)
    dense[1:7] = rng.poisson(400, (6, V)) + 200
    dense[1:7, -20:] += 500      # the same columns lead in every row
    dense[7:] = rng.poisson(30, (2, V))
    dense[7:, V // 2:] += 600      # the upper half binds the antigen: q3 + 3 iqr passes 1000
    dense[7:, V - 1] += 4000
    fx = R.from_dense(dense, _kinds(1, 6, 2))
    ref = R.remove_aggregates(fx, "high")
    n_agg = int((ref["reasons"] & R.COUNTS != 0).sum())
    assert n_agg == V if V <= 25 else min(V - 6, 20) <= n_agg <= 25
    assert ref["antigen_threshold"] >= 1000 and V - 1 in ref["removed"]
    c = _ctx()
    m = _matrix(c, fx)
    _same(c, m, fx, ref)
    m.free()


@pytest.mark.parametrize("n_signal", [4, 5])
def test_four_and_five_signal_antibodies(n_signal):
    """five antibody rows, one of them with a sum of 999 (4 signal antibodies: nothing runs) or exactly 1000 (5: all five needed)"""
    rng = np.random.RandomState(9)
    V = 300
    dense = np.zeros((6, V), np.int64)
    dense[1:] = rng.poisson(20, (5, V))
    dense[1:, [5, 17, 250]] = 900
    dense[3] = 0
    dense[3, [5, 17, 250]] = 300
    dense[3, 100] = 99 if n_signal == 4 else 100
    fx = R.from_dense(dense, _kinds(1, 5))
    ref = R.remove_aggregates(fx, "high")
    assert ref["info"]["n_signal"] == n_signal and list(ref["removed"]) == ([] if n_signal == 4 else [5, 17, 250])
    assert ref["info"]["n_candidates"] == (0 if n_signal == 4 else 25)
    c = _ctx()
    m = _matrix(c, fx)
    _same(c, m, fx, ref)
    m.free()


@pytest.mark.parametrize("lds", LDS)
def test_seventy_signal_antibodies_more_than_a_waves_round_per_column(lds):
    """70 signal antibodies (frac = 0.6: 42 needed): the planted columns hold more than 64 antibody entries, a second round of the wave"""
    fx = R.random_well(31, n_ab=70, V=700, n_gex=40)
    ref = R.remove_aggregates(fx, "high")
    assert ref["info"]["n_signal"] == 70 and ref["info"]["min_antibodies"] == 42
    col = np.repeat(np.arange(700), np.diff(fx["indptr"]))
    assert np.bincount(col[fx["kind"][fx["indices"]] == R.KIND_ANTIBODY]).max() > 64
    assert (ref["reasons"] & R.COUNTS != 0).sum() >= 2
    assert np.array_equal(ref["removed"], R.remove_aggregates(fx, "low")["removed"])
    c = _ctx(lds)
    m = _matrix(c, fx)
    _same(c, m, fx, ref, lds)
    m.free()


@pytest.mark.parametrize("lds", [None, "4096", "3"])
def test_a_table_too_wide_for_one_slice(lds):
    """K = 400 and 70 signal rows: 336 KB of pairs and counters.  By default the table then stays in device memory; asked for, it is
    cut into slices of 34 rows (3 slices, the last one of 2 rows)"""
    fx = dict(R.random_well(31, n_ab=70, V=700, n_gex=40), num_probe_barcodes=16)
    ref = _ref("wide", fx)
    assert ref["info"]["top_k"] == ref["info"]["n_candidates"] == 400 and (ref["reasons"] & R.COUNTS != 0).sum() >= 2
    c = _ctx(lds)
    m = _matrix(c, fx)
    agg = _same(c, m, fx, ref, "0" if lds is None else lds)
    if lds == "4096":
        assert (agg.info["rows_per_slice"], agg.info["n_slices"]) == (34, 3)
    m.free()


@pytest.mark.parametrize("lds", LDS)
def test_antibody_rows_interleaved_with_other_rows(lds):
    """the antibody rows are no contiguous range: a slice's feature range holds rows of other kinds and of other slices"""
    fx = R.random_well(47, n_ab=17, V=900, n_gex=30, n_ag=3, interleave=True, num_probe_barcodes=2)
    ab = np.flatnonzero(fx["kind"] == R.KIND_ANTIBODY)
    assert (np.diff(ab) > 1).sum() >= 5
    ref = R.remove_aggregates(fx, "high")
    assert ref["info"]["top_k"] == 50 and (ref["reasons"] & R.COUNTS != 0).sum() >= 1
    c = _ctx(lds)
    m = _matrix(c, fx)
    _same(c, m, fx, ref, lds, check_matrix=True)
    m.free()


# ---- highly corrected barcodes, the union --------------------------------------------------------------------------------------------
def test_highly_corrected_at_the_thresholds():
    from cellranger_amd import _lib

    c = _ctx()
    reads = np.array([10000, 10001, 10001, 10002, 10002, 20000, 20000, 0, 4000000000, 4000000000], np.uint32)
    corr = np.array([10000, 5000, 5001, 5001, 5002, 10000, 10001, 0, 2000000000, 2000000001], np.uint32)
    exp = R.highly_corrected(reads, corr)
    assert list(exp) == [2, 4, 6, 9]      # 10000 reads are not enough; 2 * corrected == reads is not above one half
    reasons = c.zeros(len(reads), np.uint8)
    assert c.highly_corrected(c.upload(reads), c.upload(corr), reasons) == len(exp)
    assert np.array_equal(np.flatnonzero(reasons.to_host() == _lib.AGG_HIGHLY_CORRECTED), exp.astype(np.int64))
    with pytest.raises(ValueError):
        c.highly_corrected(c.upload(reads), c.upload(corr[:5]), reasons)


def test_union_reason_bits_and_disable():
    """column 70 of the sparse-row fixture is caught by its counts and by its corrected reads, column 1 only by the reads.
    disable=True reports the same and returns the matrix itself"""
    fx = _sparse_row_fixture()
    V = len(fx["indptr"]) - 1
    reads = np.full(V, 500, np.uint32)
    corr = np.full(V, 10, np.uint32)
    reads[[1, 70]], corr[[1, 70]] = 20000, 15000
    fx = dict(fx, reads={R.AB: reads}, corrected={R.AB: corr})
    ref = R.remove_aggregates(fx, "high")
    assert list(ref["removed"]) == [1, 70, 75, 78] and list(ref["reasons"]) == [2, 3, 1, 1]
    assert ref["libraries"][R.AB]["reads_removed"] == 41000 and ref["libraries"][R.AB]["reads_total"] == 78 * 500 + 40000
    c = _ctx()
    m = _matrix(c, fx)
    _same(c, m, fx, ref, check_matrix=True)
    same, agg = c.remove_aggregates(m, fx["kind"], reads=fx["reads"], corrected_reads=fx["corrected"], disable=True)
    assert same is m and agg.disabled and np.array_equal(agg.removed_cols, ref["removed"]) and list(agg.cols_with(2)) == [1, 70]
    m.free()


# ---- Counts.corrected_reads_per_column ------------------------------------------------------------------------------------------------
def test_corrected_reads_per_column_of_a_counted_well():
    import gpu_helpers as G
    from cellranger_amd import engine as E
    from cellranger_amd import synth as S

    n = 6000
    w = S.Workload(n_total=n, seed=21, n_wl=2000, n_cells=30, n_ambient=200, n_genes=20, umi_len=5, umi_err=0.08, cb_err=0.01, reads_per_umi=3, n_libs=2)
    c = G.fresh_ctx()
    for lib in range(2):
        c.set_whitelist(lib, w.wl_packed, length=16)
    r = w.host_reads(0, n)
    _, _, _, dev = G.gpu_barcode_stage(c, r, n)
    c.set_key_layout(w.n_genes, w.umi_len, 2, 0)
    d = [c.upload(r["umi"]), c.upload(r["umi_qualn"]), c.upload(r["feature"])]
    recs = c.records(n, w.umi_len, dev["idx"], d[0], d[1], d[2], dev["flags"])
    counts = c.count_records(recs)
    raw = c.assemble_matrix_dev(*counts.triplets_dev(), counts.n_triplets)
    rank = raw.download()[0]
    rows = counts.barcode_summary()
    assert rows["umi_corrected_reads"].sum() > 0 and set(rows["library"]) == {0, 1}
    for libs in (0, 1, (0, 1)):
        exp = np.zeros(int(rank.max()) + 1, np.uint64)
        sel = np.isin(rows["library"], libs)
        np.add.at(exp, rows["barcode_rank"][sel][rows["barcode_rank"][sel] <= rank.max()], rows["umi_corrected_reads"][sel][rows["barcode_rank"][sel] <= rank.max()])
        got = counts.corrected_reads_per_column(raw, libs).to_host()
        assert np.array_equal(got, exp[rank].astype(np.uint32)), libs
    with pytest.raises(E.CrgpuError) as e:
        counts.corrected_reads_per_column(raw, 5)      # beyond the two libraries of the key layout
    assert e.value.code == EINVAL
    # counts made from bare keys carry no table
    d_keys = c.empty(n, np.uint64)
    bare = c.count_keys(d_keys, c.build_keys(recs, d_keys))
    if bare.n_molecules:
        with pytest.raises(E.CrgpuError) as e:
            bare.corrected_reads_per_column(raw, 0)
        assert e.value.code == ESTATE and "corrected-read table" in str(e.value)
    c.close()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    import ctypes as C

    from cellranger_amd import _lib
    from cellranger_amd import engine as E

    c = _ctx()
    fx = _sparse_row_fixture()
    m = _matrix(c, fx)
    for bad in (fx["kind"][:-1], np.append(fx["kind"][:-1], 3)):      # a row >= n_features; a kind that is none
        with pytest.raises(E.CrgpuError) as e:
            c.remove_aggregates(m, bad)
        assert e.value.code == EINVAL
    with pytest.raises(E.CrgpuError) as e:
        c.aggregates_by_counts(m, fx["kind"], num_probe_barcodes=41)
    assert e.value.code == ERANGE
    with pytest.raises(ValueError):
        c.remove_aggregates(m, fx["kind"], reads={R.AB: np.zeros(5, np.uint32)})
    # rows that do not ascend: a view built by hand, one column whose first two rows are swapped
    d = [c.upload(np.zeros(1, np.uint32)), c.upload(np.array([0, 8], np.int64)), c.upload(np.array([1, 0, 2, 3, 4, 5, 6, 7], np.int32)),
         c.upload(np.full(8, 500, np.int32))]
    view = _lib.MatrixDevView(1, 8, d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr)
    mv = E.MatrixDev(c, C.pointer(view))
    try:
        with pytest.raises(E.CrgpuError) as e:
            c.aggregates_by_counts(mv, fx["kind"])
        assert e.value.code == EINVAL and "ascend" in str(e.value)
    finally:
        mv._mv = None      # the view is this test's: nothing to release through crgpu_matrix_dev_free
    # column lists
    umis = c.column_sums(m)
    call = c.call_cells_ordmag(m, force_cells=10)
    V = m.n_barcodes
    for cols in (np.arange(V + 1), np.array([3, 1]), np.array([1, 1]), np.array([0, V])):      # longer than V, not ascending, repeated, out of range
        bad_call = E.CellCall(c, c.upload(cols.astype(np.uint64)), len(cols), dict(call.metrics), m)
        with pytest.raises(E.CrgpuError) as e:
            c.apply_minimum_umis(bad_call, umis, 1)
        assert e.value.code == EINVAL
        with pytest.raises(E.CrgpuError) as e:
            c.apply_mito_threshold(bad_call, umis, umis, 5.0)
        assert e.value.code == EINVAL
    with pytest.raises(E.CrgpuError) as e:
        c.take_columns(umis, np.array([V], np.uint64))
    assert e.value.code == EINVAL
    m.free()
