"""The two closing filters of a cell call on the device (Context.apply_minimum_umis, Context.apply_mito_threshold) against the
restatement tests/aggregates_numpy.py: equality, the order of the call preserved, and the result accepted by Context.matrix_summary."""
import numpy as np
import pytest

import aggregates_numpy as R
from aggregates_gpu import ctx as _ctx, matrix as _matrix

pytestmark = pytest.mark.gpu
_shared = {}


def _well():
    """500 columns x 40 Gene Expression rows, rows 0 .. 4 mitochondrial; 300 called cells.  Some cells have no count at all (0 / 0),
    some sit exactly at 10 % (2 of 20)"""
    if "well" not in _shared:
        rng = np.random.RandomState(12)
        V = 500
        dense = rng.poisson(3.0, (40, V))
        dense[:5] = rng.poisson(1.2, (5, V))
        dense[:, 7::50] = 0                      # empty columns: NaN
        dense[:, 11::50] = 0
        dense[0, 11::50], dense[20, 11::50] = 2, 18      # exactly 10.0 %
        fx = R.from_dense(dense, np.zeros(40, np.uint8))
        mito = np.zeros(40, bool)
        mito[:5] = True
        cells = np.sort(rng.choice(V, 300, replace=False))
        cells = np.union1d(cells, np.arange(7, V, 50)[:4]).astype(np.uint64)
        cells = np.union1d(cells, np.arange(11, V, 50)[:4]).astype(np.uint64)
        c = _ctx()
        m = _matrix(c, fx)
        _shared["well"] = (c, m, fx, mito, cells, c.column_sums(m), c.column_sums(m, mito),
                           R.column_sums(fx["indptr"], fx["indices"], fx["data"], np.ones(40, bool)), R.column_sums(fx["indptr"], fx["indices"], fx["data"], mito))
    return _shared["well"]


def _call(c, m, cells):
    from cellranger_amd import engine as E

    return E.CellCall(c, c.upload(cells), len(cells), {"filtered_bcs": len(cells)}, m)


@pytest.mark.parametrize("minimum", [0, 1, 100, 118, 119, 10 ** 6])
def test_minimum_umis(minimum):
    c, m, fx, mito, cells, d_tot, d_mt, tot, mt = _well()
    exp = R.apply_minimum_umis(cells, tot, minimum)
    assert len(exp) == len(cells) if minimum == 0 else len(exp) < len(cells)
    assert len(exp) == 0 if minimum == 10 ** 6 else len(exp) > 0
    out = c.apply_minimum_umis(_call(c, m, cells), d_tot, minimum)
    assert out.n_cells == len(exp) and np.array_equal(out.cols_host(), exp)
    assert out.metrics == {"filtered_bcs": len(cells)}
    # a numpy array of UMIs serves as well
    assert np.array_equal(c.apply_minimum_umis(_call(c, m, cells), tot.astype(np.uint32), minimum).cols_host(), exp)


@pytest.mark.parametrize("max_pct", [100.0, 10.0, 5.0, 4.999, 0.0, -1.0])
def test_mito_threshold(max_pct):
    c, m, fx, mito, cells, d_tot, d_mt, tot, mt = _well()
    kept, removed, r_tot, r_pct = R.apply_mito_threshold(cells, mt, tot, max_pct)
    nan_cells = cells[tot[cells.astype(np.int64)] == 0]
    assert len(nan_cells) >= 4 and np.isin(nan_cells, kept).all()      # 0 / 0 stays whatever the threshold
    if max_pct == 100.0:
        assert len(removed) == 0
    if max_pct == 10.0:
        assert np.isin(np.arange(11, 500, 50)[:4], kept).all() and len(removed) > 0      # exactly at the threshold: stays
    if max_pct == -1.0:
        assert np.array_equal(kept, nan_cells)      # everything with a percentage leaves
    out, summary = c.apply_mito_threshold(_call(c, m, cells), d_mt, d_tot, max_pct)
    assert out.n_cells == len(kept) and np.array_equal(out.cols_host(), kept)
    assert np.array_equal(summary["cols"], removed) and np.array_equal(summary["total_umis"], r_tot.astype(np.uint32))
    assert summary["mt_pct"].tobytes() == r_pct.tobytes() and summary["threshold"] == max_pct


def test_filtered_calls_feed_the_later_stages():
    """both results are CellCalls that matrix_summary, filtered_matrix and remove_high_occupancy_gems' column lists accept"""
    c, m, fx, mito, cells, d_tot, d_mt, tot, mt = _well()
    call = c.apply_minimum_umis(_call(c, m, cells), d_tot, 100)
    call, _ = c.apply_mito_threshold(call, d_mt, d_tot, 5.0)
    exp = R.apply_mito_threshold(R.apply_minimum_umis(cells, tot, 100), mt, tot, 5.0)[0]
    assert 0 < call.n_cells < len(cells) and np.array_equal(call.cols_host(), exp)
    s = c.matrix_summary(m, call, n_features=40)
    assert s.classes[0]["n_cells"] == len(exp) and s.classes[0]["cells_total_counts"] == int(tot[exp.astype(np.int64)].sum())
    f = call.filtered_matrix()
    assert f.n_barcodes == len(exp) and np.array_equal(f.download()[0], exp.astype(np.uint32))
    f.free()
    # an empty call goes through both filters
    empty = _call(c, m, np.zeros(0, np.uint64))
    assert c.apply_minimum_umis(empty, d_tot, 5).n_cells == 0
    out, summary = c.apply_mito_threshold(empty, d_mt, d_tot, 5.0)
    assert out.n_cells == 0 and len(summary["cols"]) == 0
