"""The filtered-matrix summary on the device (Context.matrix_summary -> crgpu_matrix_summary_dev, Context.reads_per_column,
engine.matrix_summary_metrics) against the restatement tests/matrix_summary_numpy.py, which tests/test_matrix_summary_restatement.py
pins against the reference's recorded outputs.  Every integer and every float is compared for equality (floats as bit patterns, NaN
equal to NaN); the standard deviation within 4 ulp of the exact value and cv = std / mean within 5 * 2^-52 relative, as
tests/test_matrix_summary_abi.py holds the host function.  Matrices are built as tests/test_gpu_emptydrops.py::_matrix builds them:
column k is whitelist entry k."""
import math
import os

import numpy as np
import pytest

import matrix_summary_numpy as R
from test_matrix_summary_abi import _same_floats

pytestmark = pytest.mark.gpu
WL = 131072
EINVAL, ERANGE = -1, -6
LIST_FIELDS = ("counts_q", "genes_q", "top_counts_feature", "top_counts_value", "top_cells_feature", "top_cells_value")
_shared = {}


def _ctx(fresh=False):
    import gpu_helpers as G

    if fresh or "ctx" not in _shared:
        c = G.fresh_ctx()
        c.set_whitelist(0, np.arange(WL, dtype=np.uint32), length=16)      # rank == value: column k is barcode k
        if fresh:
            return c
        _shared["ctx"] = c
    return _shared["ctx"]


def _matrix(c, fx):
    """MatrixDev of a fixture; the read table goes into the VALID counts of library 0 (every column keeps a non-zero entry there)"""
    indptr, V = fx["indptr"], len(fx["indptr"]) - 1
    seen = np.zeros(c.n_canon, np.uint32)
    seen[:V] = 1 if fx["reads"] is None else np.maximum(fx["reads"], 1)
    c.set_counts(0, 0, seen)
    c.set_counts(0, 1, np.zeros(c.n_canon, np.uint32))
    bc = np.repeat(np.arange(V, dtype=np.uint32), np.diff(indptr))
    m = c.assemble_matrix_dev(c.upload(bc), c.upload(fx["indices"].astype(np.uint32)), c.upload(fx["data"].astype(np.uint32)), len(bc))
    assert m.n_barcodes == V and m.nnz == len(bc)
    return m


def _same(s, ref, fx, per_cell=True):
    """a MatrixSummary against R.summary: integers, lists, floats, the optional device arrays"""
    assert np.array_equal(s.counts_per_feature, ref["counts_per_feature"]) and np.array_equal(s.cells_ge2_per_feature, ref["cells_ge2_per_feature"])
    have = fx["reads"] is not None
    assert (s.reads_all, s.reads_union) == ((ref["reads_all"], ref["reads_union"]) if have else (None, None))
    assert s.n_classes == ref["n_classes"] and s.n_listed == len(fx["cells"])
    for k, (got, exp) in enumerate(zip(s.classes, ref["classes"])):
        for name in R.CLASS_INT_FIELDS + ("n_top",) + LIST_FIELDS:
            assert got[name] == exp[name], (k, name, got[name], exp[name])
        _same_floats(s.floats(k), R.class_floats(exp, exp["reads_cells"], ref["reads_all"]))
    if per_cell:
        assert np.array_equal(s.counts_per_cell.to_host(), ref["counts_per_cell"].astype(np.uint32))
        assert np.array_equal(s.genes_per_cell.to_host(), ref["genes_per_cell"].astype(np.uint32))


def _run(c, m, fx, **kw):
    args = dict(feature_class=fx["feature_class"], n_classes=fx["n_classes"], cell_class_mask=fx["cell_class_mask"], reads=fx["reads"], per_cell=True)
    args.update(kw)
    return c.matrix_summary(m, fx["cells"], **args)


def _mid():
    if "mid" not in _shared:
        fx = R.make_matrix(11)
        _shared["mid"] = (fx, R.run(fx))
    return _shared["mid"]


# ---- the fixtures ------------------------------------------------------------------------------------------------------------------
def test_hand_matrix():
    c, fx = _ctx(), R.hand_matrix()
    m = _matrix(c, fx)
    s = _run(c, m, fx)
    _same(s, R.run(fx), fx)
    assert s.classes[1]["top_counts_feature"] == [4, 3] and s.classes[1]["top_counts_value"] == [8, 3] and s.classes[0]["counts_q"] == [6] * 6
    # one class over every feature, a cell of every class by default: feature_class and cell_class_mask left out
    one = c.matrix_summary(m, fx["cells"], n_features=6)
    ref = R.summary(fx["indptr"], fx["indices"], fx["data"], 6, fx["cells"])
    fx1 = dict(fx, reads=None)
    _same(one, ref, fx1, per_cell=False)
    assert one.counts_per_cell is None and one.classes[0]["raw_total_counts"] == int(fx["data"].sum())


@pytest.mark.parametrize("lds", [None, "64", "7", "0"])
def test_mid_matrix_in_every_slice_form(lds):
    """300 features x 1000 columns, three classes and features of none, overlapping cell masks; CRGPU_MS_LDS_FEATURES is read when a
    context is created: several slices (64: 5, 7: 43), one slice (unset), counters in device memory (0).  The results are the same."""
    fx, ref = _mid()
    old = os.environ.pop("CRGPU_MS_LDS_FEATURES", None)
    try:
        if lds is not None:
            os.environ["CRGPU_MS_LDS_FEATURES"] = lds
        c = _ctx(fresh=True)
    finally:
        os.environ.pop("CRGPU_MS_LDS_FEATURES", None)
        if old is not None:
            os.environ["CRGPU_MS_LDS_FEATURES"] = old
    m = _matrix(c, fx)
    _same(_run(c, m, fx), ref, fx)
    m.free()
    c.close()


@pytest.mark.parametrize("big", [False, True])
def test_wave_loop_columns_and_a_feature_of_every_cell(big):
    """empty columns, columns of 65 and 300 entries, feature 7 in every cell; big: data up to 2^31 - 1, the sum of feature 7 passes 2^32
    and so does the share of one workgroup: its u32 LDS counter wraps and carries, while every per-cell sum stays below 2^32"""
    c, fx = _ctx(), R.wave_matrix(big)
    ref = R.run(fx)
    assert np.diff(fx["indptr"]).max() == 300 and 65 in np.diff(fx["indptr"]) and (np.diff(fx["indptr"]) == 0).sum() >= 4
    assert (int(ref["counts_per_feature"][7]) > 2 ** 32) == big and ref["cells_ge2_per_feature"][7] >= (6 if big else 0)
    assert max(int(x.max()) for x in ref["counts_per_cell"]) < 2 ** 32
    # the pass gives a workgroup every G-th group of 16 columns; 64 columns are 4 groups, one per workgroup.  The share of feature 7
    # (class 1) that one workgroup adds to its u32 counter, from the fixture itself:
    col = np.repeat(np.arange(64), np.diff(fx["indptr"]))
    own = np.zeros(64, bool)
    own[fx["cells"][(fx["cell_class_mask"] >> 1) & 1 == 1].astype(np.int64)] = True
    take = (fx["indices"] == 7) & own[col]
    share = np.bincount(col[take] // 16, weights=fx["data"][take].astype(np.float64), minlength=4)
    assert (share.max() >= 2 ** 32) == big and share.sum() == int(ref["counts_per_feature"][7])
    _same(_run(c, _matrix(c, fx), fx), ref, fx)


def test_many_columns_several_workgroups_per_slice():
    """70 000 columns, ~1 M entries, 4 classes in 600 features: grid-stride loops over the columns, several slab rows"""
    fx = R.make_matrix(23, n_features=600, n_cols=70000, entries=12, n_cells=3000, n_classes=4, max_count=300)
    assert 900_000 < len(fx["indices"]) < 1_400_000
    c = _ctx()
    _same(_run(c, _matrix(c, fx), fx), R.run(fx), fx)


def test_more_than_four_classes():
    """the 32-class instantiation of the pass: 9 classes, cells of several"""
    fx = R.make_matrix(31, n_features=200, n_cols=400, entries=15, n_cells=60, n_classes=9)
    c = _ctx()
    _same(_run(c, _matrix(c, fx), fx), R.run(fx), fx)


# ---- edge cases and refusals --------------------------------------------------------------------------------------------------------
def test_no_cells_an_empty_class_and_an_empty_matrix():
    from cellranger_amd import engine as E

    c, fx = _ctx(), R.hand_matrix()
    m = _matrix(c, fx)
    none = np.zeros(0, np.uint64)
    s = c.matrix_summary(m, none, feature_class=fx["feature_class"], n_classes=2, reads=fx["reads"], per_cell=True)
    ref = R.summary(fx["indptr"], fx["indices"], fx["data"], 6, none, fx["feature_class"], 2, np.zeros(0, np.uint32), fx["reads"])
    _same(s, ref, dict(fx, cells=none))
    assert s.classes[0]["raw_total_counts"] == 35 and s.classes[0]["n_cells"] == 0 and math.isnan(s.floats(0)["counts_mean"])
    assert E.matrix_summary_metrics(s, 0, "GRCh38", list("abcdef")) == {}
    # a class without cells: zeros, n_cells 0; the third cell is listed and of no class
    mask = np.array([1, 1, 0], np.uint32)
    s = _run(c, m, fx, cell_class_mask=mask)
    _same(s, R.run(fx, cell_class_mask=mask), dict(fx, cell_class_mask=mask))
    assert s.classes[1]["n_cells"] == 0 and s.classes[1]["cells_total_counts"] == 0 and s.classes[1]["union_total_counts"] == 18
    # a matrix without entries: three columns, two of them cells
    seen = np.zeros(c.n_canon, np.uint32)
    seen[[5, 17, 900]] = 1
    c.set_counts(0, 0, seen)
    z = np.zeros(0, np.uint32)
    empty = c.assemble_matrix_dev(c.upload(z), c.upload(z), c.upload(z), 0)
    s = c.matrix_summary(empty, np.array([0, 2], np.uint64), n_features=6, per_cell=True)
    assert not s.counts_per_feature.any() and s.classes[0]["n_cells"] == 2 and s.classes[0]["counts_q"] == [0] * 6
    assert s.floats(0)["counts_mean"] == 0.0 and math.isnan(s.floats(0)["counts_cv"]) and not s.counts_per_cell.to_host().any()
    # a matrix without columns: the same zeros and the same top features (ties by feature index) as the raw matrix without cells
    nothing = E.CellCall(c, c.empty(0, np.uint64), 0, {"filtered_bcs": 0}, m).filtered_matrix()
    assert nothing.n_barcodes == 0
    s0 = c.matrix_summary(nothing, none, feature_class=fx["feature_class"], n_classes=2)
    s1 = c.matrix_summary(m, none, feature_class=fx["feature_class"], n_classes=2)
    for a, b in zip(s0.classes, s1.classes):
        assert dict(a, raw_total_counts=0) == dict(b, raw_total_counts=0) and a["raw_total_counts"] == 0
    assert s0.classes[0]["top_counts_feature"] == [0, 1, 2] and s0.classes[1]["top_cells_feature"] == [3, 4] and s0.classes[1]["top_cells_value"] == [0, 0]


def test_refusals():
    from cellranger_amd import engine as E

    c, fx = _ctx(), R.hand_matrix()
    m = _matrix(c, fx)
    for cells in ([3, 1, 6], [1, 1, 6], [1, 3, 8]):      # not ascending, repeated, out of range
        with pytest.raises(E.CrgpuError) as e:
            c.matrix_summary(m, np.array(cells, np.uint64), n_features=6)
        assert e.value.code == EINVAL
    with pytest.raises(E.CrgpuError) as e:
        c.matrix_summary(m, fx["cells"], n_features=5)      # row 5 >= n_features
    assert e.value.code == EINVAL and "row" in str(e.value)
    for bad in (dict(feature_class=np.array([0, 0, 2, 1, 1, 0xFF], np.uint8), n_classes=2), dict(n_features=6, n_classes=0), dict(n_features=6, n_classes=33)):
        with pytest.raises(E.CrgpuError) as e:
            c.matrix_summary(m, fx["cells"], **bad)
        assert e.value.code == EINVAL
    # a per-cell sum past 32 bits: three entries of 2^31 - 1 in one cell
    big = dict(fx, data=fx["data"].copy())
    big["data"][fx["indptr"][3]: fx["indptr"][3] + 3] = 2 ** 31 - 1
    mb = _matrix(c, big)
    with pytest.raises(E.CrgpuError) as e:
        c.matrix_summary(mb, fx["cells"], n_features=6)
    assert e.value.code == ERANGE
    s = c.matrix_summary(mb, np.array([1, 6], np.uint64), n_features=6)      # ... which is no cell here: the 64-bit totals hold
    assert s.classes[0]["raw_total_counts"] == int(big["data"].astype(np.int64).sum())


def test_rows_that_do_not_ascend_are_refused():
    """the slice search relies on ascending rows; the pass counts the entries it looked at, and a count short of nnz is CRGPU_EINVAL.  A
    view built by hand: one column of 100 entries, rows 0 .. 99 with the first and the last swapped, two slices of 50 features.  The
    search of slice 0 stops at position 48 and that of slice 1 starts there: 96 of the 100 entries are found (worked out by replaying
    the 64-ary search on the CPU).  With one slice nothing is searched and the sums, which do not depend on the order, are reported."""
    import ctypes as C

    from cellranger_amd import _lib
    from cellranger_amd import engine as E

    rows = np.arange(100, dtype=np.int32)
    rows[0], rows[99] = 99, 0
    data = np.arange(1, 101, dtype=np.int32)
    for lds, refused in (("50", True), (None, False)):
        old = os.environ.pop("CRGPU_MS_LDS_FEATURES", None)
        try:
            if lds is not None:
                os.environ["CRGPU_MS_LDS_FEATURES"] = lds
            c = _ctx(fresh=True)
        finally:
            os.environ.pop("CRGPU_MS_LDS_FEATURES", None)
            if old is not None:
                os.environ["CRGPU_MS_LDS_FEATURES"] = old
        d = [c.upload(np.zeros(1, np.uint32)), c.upload(np.array([0, 100], np.int64)), c.upload(rows), c.upload(data)]
        view = _lib.MatrixDevView(1, 100, d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr)
        m = E.MatrixDev(c, C.pointer(view))
        try:
            if refused:
                with pytest.raises(E.CrgpuError) as e:
                    c.matrix_summary(m, np.array([0], np.uint64), n_features=100)
                assert e.value.code == EINVAL and "ascend" in str(e.value) and "96 of 100" in str(e.value)
            else:
                s = c.matrix_summary(m, np.array([0], np.uint64), n_features=100)
                assert s.classes[0]["cells_total_counts"] == 5050 and s.counts_per_feature[99] == 1 and s.counts_per_feature[0] == 100
        finally:
            m._mv = None      # the view is this test's, not the library's: nothing to release through crgpu_matrix_dev_free
        c.close()


# ---- reads per column ---------------------------------------------------------------------------------------------------------------
def test_reads_per_column_against_the_histograms():
    from cellranger_amd import engine as E

    c = _ctx(fresh=True)
    c.set_whitelist(1, np.arange(WL, dtype=np.uint32), length=16)
    rng = np.random.RandomState(4)
    tabs = {}
    for lib in (0, 1):
        for which in (0, 1):
            t = np.zeros(c.n_canon, np.uint32)
            t[rng.choice(5000, 700, replace=False)] = rng.randint(1, 10 ** 6, 700)
            c.set_counts(lib, which, t)
            tabs[lib, which] = t
    z = np.zeros(0, np.uint32)
    m = c.assemble_matrix_dev(c.upload(z), c.upload(z), c.upload(z), 0)
    rank = m.download()[0]
    down = {k: c.get_counts(*k) for k in tabs}      # the downloaded histograms
    assert all(np.array_equal(down[k], tabs[k]) for k in tabs) and len(rank) > 1500
    for libs, use in ((0, (0,)), ([1], (1,)), ([0, 1], (0, 1))):
        exp = sum(down[l, w][rank].astype(np.uint64) for l in use for w in (0, 1))
        assert np.array_equal(c.reads_per_column(m, libs).to_host(), exp.astype(np.uint32))
    for libs in ([2], [0, 5]):      # no whitelist for the library
        with pytest.raises(E.CrgpuError) as e:
            c.reads_per_column(m, libs)
        assert e.value.code == EINVAL
    for which in (0, 1):      # 2 (2^32 - 1) reads on one barcode
        t = tabs[0, which].copy()
        t[rank[3]] = 0xFFFFFFFF
        c.set_counts(0, which, t)
    with pytest.raises(E.CrgpuError) as e:
        c.reads_per_column(m, [0, 1])
    assert e.value.code == ERANGE
    c.close()


# ---- a real count -> cell call run ---------------------------------------------------------------------------------------------------
def test_metrics_of_a_counted_and_called_well():
    import gpu_helpers as G
    from cellranger_amd import engine as E
    from cellranger_amd import synth as S

    n = 200_000
    w = S.Workload(n_total=n, seed=S.SEED0 + 5, n_wl=100_000, n_cells=200, n_ambient=10_000, n_genes=2000)
    r = w.host_reads(0, n)
    c = G.fresh_ctx()
    c.set_whitelist(0, w.wl_packed, length=16)
    _, _, _, dev = G.gpu_barcode_stage(c, r, n)
    c.set_key_layout(w.n_genes, w.umi_len, 1, 0)
    d = [c.upload(r["umi"]), c.upload(r["umi_qualn"]), c.upload(r["feature"])]
    counts = c.count_records(c.records(n, w.umi_len, dev["idx"], d[0], d[1], d[2], dev["flags"]))
    raw = c.assemble_matrix_dev(*counts.triplets_dev(), counts.n_triplets)
    call = c.call_cells_ordmag(raw)
    assert 50 < call.n_cells < raw.n_barcodes
    # two genomes by feature parity, every 50th feature in neither; a cell is of the genome that holds most of its counts
    fc = (np.arange(w.n_genes) % 2).astype(np.uint8)
    fc[::50] = R.NO_CLASS
    rank, indptr, indices, data = raw.download()
    cells = call.cols_host()
    sums = [np.asarray(R.sum_masked(indptr, indices, data.astype(np.int64), w.n_genes, fc == g, np.ones(len(rank), bool), 0))[cells.astype(np.int64)]
            for g in (0, 1)]
    mask = np.where(sums[0] >= sums[1], 1, 2).astype(np.uint32)
    mask[::7] = 3
    reads = c.reads_per_column(raw, 0)
    h_reads = (c.get_counts(0, 0)[rank].astype(np.uint64) + c.get_counts(0, 1)[rank]).astype(np.uint32)
    assert np.array_equal(reads.to_host(), h_reads) and h_reads.sum() > data.sum()
    s = c.matrix_summary(raw, call, feature_class=fc, n_classes=2, cell_class_mask=mask, reads=reads)
    fx = dict(indptr=indptr, indices=indices, data=data, n_features=w.n_genes, n_classes=2, feature_class=fc, cells=cells, cell_class_mask=mask, reads=h_reads)
    _same(s, R.run(fx), fx, per_cell=False)
    ids = ["ENSG%08d" % f for f in range(w.n_genes)]
    for k, genome in enumerate(("GRCh38", "mm10")):
        got = E.matrix_summary_metrics(s, k, genome, ids, total_reads=n, conf_mapped_reads=int(h_reads.sum()), recovered_cells=150)
        ref = R.report(indptr, indices, data, w.n_genes, cells, k, genome, ids, fc, 2, mask, h_reads, total_reads=n, conf_mapped_reads=int(h_reads.sum()),
                       recovered_cells=150)
        assert sorted(got) == sorted(ref) and len(got) > 30
        for key, v in ref.items():
            if key.endswith("_cv_counts") or key.endswith("_cv_unique_genes_detected"):      # np.std on the reference's side
                assert abs(got[key] - v) <= (64 * 2.0 ** -53 + 2 * 2.0 ** -53) * v, key
            elif isinstance(v, float):
                assert (math.isnan(v) and math.isnan(got[key])) or np.float64(got[key]).view(np.uint64) == np.float64(v).view(np.uint64), (key, got[key], v)
            else:
                assert got[key] == v, (key, got[key], v)
    c.close()
