"""GPU tests of the EmptyDrops step on a well that can be written down by hand (tests/cpp/test_emptydrops.cpp holds the same well).

1023 features; feature classes r = 1 .. 10 of 2^(10 - r) features each.  Ambient column k (k = 1 .. 10) holds one count of every
feature of a class >= k, so the ambient row sum of a feature of class r is r: ten distinct frequencies, frequency r occurring
2^(10 - r) times, and NO feature of the matrix is missing from the ambient set -- the profile has no zero class and is pstar
renormalised (cell_calling.py:68-70), the branch the planted wells never reach.  Column 10 holds 3 r counts of every feature (the
profile's shape: about the likeliest vector of its total), column 11 holds 2000 counts of one class-1 feature (nothing like the
profile), column 12 is the one initial cell.  Descending totals: 50000, 6108, 2000, 1023, 511, .., 1 -- no ties."""
import ctypes as C

import numpy as np
import pytest

import emptydrops_numpy as R
from test_gpu_emptydrops import _check_calls, _check_floats, _check_integers, _ctx, _initial, _matrix, _table_close

pytestmark = pytest.mark.gpu
F = 1023
LOW, HIGH, MIN_UMIS, SIMS = 3, 13, 5, 200


def hand_well():
    cls = np.concatenate([np.full(1 << (10 - r), r) for r in range(1, 11)])
    cols = [np.arange(1024 - (1 << (11 - k)), F) for k in range(1, 11)]
    cols = [(f, np.ones(len(f), np.int64)) for f in cols]
    cols += [(np.arange(F), 3 * cls), (np.array([0]), np.array([2000])), (np.array([1022]), np.array([50000]))]
    indptr = np.concatenate([[0], np.cumsum([len(f) for f, _ in cols])]).astype(np.int64)
    return indptr, np.concatenate([f for f, _ in cols]).astype(np.int32), np.concatenate([x for _, x in cols]).astype(np.int32)


def test_profile_without_a_zero_class():
    indptr, indices, data = hand_well()
    cells = np.array([12])
    ref = R.find_nonambient(indptr, indices, data, F, cells, LOW, HIGH, MIN_UMIS, SIMS, 0.01, 0)
    assert ref["status"] == R.STATUS_OK and ref["n_ambient_used"] == 10 and ref["max_background_umis"] == 1023
    assert len(ref["eval_features"]) == F and np.all(R.row_sums(indptr, indices, data, F, np.arange(10)) > 0)    # no zero class
    assert np.array_equal(ref["eval_cols"], [10, 11]) and np.array_equal(ref["n_lower"], [SIMS, 0])
    c = _ctx()
    m = _matrix(c, indptr, indices, data)
    a = c.call_additional_cells(m, _initial(c, m, cells), LOW, HIGH, MIN_UMIS, num_sims=SIMS, keep_sim_table=True)
    _check_integers(a, ref)
    _check_floats(a, ref)
    assert np.array_equal(a.sim_n, ref["sim_n"]) and _table_close(a.sim_loglk, ref["sim_loglk"], ref["sim_n"])
    _check_calls(a, ref, cells, need_exact=True)
    assert np.array_equal(a.n_lower, [SIMS, 0]) and np.array_equal(a.is_nonambient, [False, True])
    assert np.array_equal(a.call.cols_host(), [11, 12])
    c.close()


def test_counts_that_are_not_the_column_sums_are_refused():
    """the observed log-likelihood takes N and the c_j from the same counts: totals that pass every range check but are not
    the sums of the (masked) columns are an error of the call, not a wrong value"""
    from cellranger_amd import _lib
    from cellranger_amd.engine import _p

    indptr, indices, data = hand_well()
    c = _ctx()
    m = _matrix(c, indptr, indices, data)
    call = _initial(c, m, np.array([12]))
    sums = R.column_sums(indptr, indices, data, F).astype(np.uint32)

    def run(counts):
        d = c.upload(counts)
        res, arr = _lib.EmptydropsResult(), _lib.EmptydropsArrays()
        rc = c.L.crgpu_emptydrops_dev(c.h, m._mv, None, 0, _p(d), _p(call.cols), 1, LOW, HIGH, MIN_UMIS, 50, 0.01, 0, None, 0, None, 0,
                                      C.byref(res), C.byref(arr))
        if rc == 0:
            c.L.crgpu_emptydrops_arrays_free(c.h, C.byref(arr))
        return rc, res.status, (c.L.crgpu_last_error(c.h) or b"").decode()

    assert run(sums)[:2] == (0, 0)
    wrong = sums.copy()
    wrong[10] -= 8                              # still a candidate, still below the largest total: only the sum can tell
    rc, _, msg = run(wrong)
    assert rc == -1 and "column sums" in msg
    assert run(sums)[:2] == (0, 0)              # the context is still usable
    c.close()
