"""The numpy restatement of the depth normalisation (tests/normalize_depth_numpy.py) against hand-computed cases (CPU).  The
reference stage (mro/rna/stages/aggregator/normalize_depth/__init__.py) imports martian and compiled extensions and cannot run
here; these tables, small enough to follow on paper, are what pins the restatement."""
import numpy as np
import pytest

import normalize_depth_numpy as N


# ---- split(): the rates -------------------------------------------------------------------------------------------------------------
def test_minimum_per_library_type_and_a_library_without_cells():
    # usable reads per cell 100, 300 (type 0) and 0 (type 1: no cells) -> the type-0 minimum is 100, the type-1 minimum 0
    frac = N.plan([0, 0, 1], [1000, 3000, 500], [10, 10, 0])
    assert np.array_equal(frac, [1.0, 100.0 / 300.0, 0.0])
    # the library without cells shares a type with another: their minimum is 0 and both keep nothing; type 1 stands alone
    frac = N.plan([0, 1, 0], [1000, 3000, 500], [10, 10, 0])
    assert np.array_equal(frac, [0.0, 1.0, 0.0])
    # the types do not see each other: 50 per cell in type 1 does not lower type 0
    assert np.array_equal(N.plan([0, 0, 1], [1000, 3000, 500], [10, 10, 10]), [1.0, 100.0 / 300.0, 1.0])


def test_targeted_adjustment_applied():
    # frac = [1, 0.25]; the targeted library 1 times 2 = 0.5 <= 1: applied
    frac = N.plan([0, 0], [1000, 4000], [10, 10], targeted_aggr=True, is_targeted_lib=[0, 1], targeted_depth_factor=2.0)
    assert np.array_equal(frac, [1.0, 0.5])
    # not a targeted aggr: the factor is not looked at
    assert np.array_equal(N.plan([0, 0], [1000, 4000], [10, 10], is_targeted_lib=[0, 1], targeted_depth_factor=2.0), [1.0, 0.25])


def test_targeted_adjustment_refused_whole():
    # 0.25 * 5 = 1.25 > 1: the unadjusted list
    frac = N.plan([0, 0], [1000, 4000], [10, 10], targeted_aggr=True, is_targeted_lib=[0, 1], targeted_depth_factor=5.0)
    assert np.array_equal(frac, [1.0, 0.25])
    # three libraries, both targeted ones fit alone (0.5 * 2, 0.25 * 2) but here library 0 (1.0 * 2) does not: nothing is adjusted
    frac = N.plan([0, 0, 0], [1000, 2000, 4000], [10, 10, 10], targeted_aggr=True, is_targeted_lib=[1, 1, 1], targeted_depth_factor=2.0)
    assert np.array_equal(frac, [1.0, 0.5, 0.25])


def test_downsample_off():
    assert np.array_equal(N.plan([0, 0, 1], [1000, 3000, 500], [10, 10, 0], downsample=False), [1.0, 1.0, 1.0])
    assert np.array_equal(N.plan([0, 0], [1000, 4000], [10, 10], downsample=False, targeted_aggr=True, is_targeted_lib=[0, 1],
                                 targeted_depth_factor=0.5), [1.0, 1.0])


# ---- main(): six molecules, rates 1 and 0: no random word decides anything -----------------------------------------------------------
#        barcode 3: feature 2 twice in library 0 and once in library 1;  barcode 5: feature 0 (library 0), feature 4 (library 1);
#        barcode 9: feature 1 (library 1).  Barcode 7 is a column without molecules.
MOL = dict(bc=np.array([3, 3, 3, 5, 5, 9]), lib=np.array([0, 0, 1, 0, 1, 1]), feature=np.array([2, 2, 2, 0, 4, 1]),
           read_count=np.array([4, 1, 7, 2, 3, 5]))
COLUMNS = np.array([3, 5, 7, 9])
FCLASS = np.array([0, 0, 0, 1, 1])            # features 3 and 4 are class 1
CELLS, CELL_MASK = np.array([5, 9]), np.array([3, 1])   # barcode 5 is a cell of both classes, barcode 9 of class 0 only


def test_six_molecules_library_0_kept():
    r = N.run(MOL, [1.0, 0.0], CELLS, COLUMNS, 5, FCLASS, 2, CELL_MASK)
    assert np.array_equal(r["kept"], [4, 1, 0, 2, 0, 0])
    # barcode 3: the two library-0 molecules of feature 2; barcode 5: feature 0; barcodes 7 and 9: empty columns
    assert np.array_equal(r["indptr"], [0, 1, 2, 2, 2]) and np.array_equal(r["indices"], [2, 0]) and np.array_equal(r["data"], [2, 1])
    assert np.array_equal(r["raw_mapped_reads"], [7, 0])          # 4 + 1 + 2 reads on class-0 features; feature 4 kept nothing
    assert np.array_equal(r["flt_mapped_reads"], [2, 0])          # barcode 5, feature 0
    assert np.array_equal(r["reads_per_lib"], [7, 15]) and np.array_equal(r["kept_reads_per_lib"], [7, 0])
    assert np.array_equal(r["kept_molecules_per_lib"], [3, 0])


def test_six_molecules_library_1_kept():
    r = N.run(MOL, [0.0, 1.0], CELLS, COLUMNS, 5, FCLASS, 2, CELL_MASK)
    assert np.array_equal(r["kept"], [0, 0, 7, 0, 3, 5])
    assert np.array_equal(r["indptr"], [0, 1, 2, 2, 3]) and np.array_equal(r["indices"], [2, 4, 1]) and np.array_equal(r["data"], [1, 1, 1])
    assert np.array_equal(r["raw_mapped_reads"], [12, 3])         # features 2 and 1: 7 + 5; feature 4: 3
    assert np.array_equal(r["flt_mapped_reads"], [5, 3])          # class 0: barcode 9 (barcode 5's feature 0 kept nothing); class 1: barcode 5
    assert np.array_equal(r["kept_reads_per_lib"], [0, 15]) and np.array_equal(r["kept_molecules_per_lib"], [0, 3])


def test_six_molecules_everything_and_nothing():
    r = N.run(MOL, [1.0, 1.0], np.zeros(0, np.int64), COLUMNS, 5)
    # one feature in both libraries of barcode 3 is one entry of three molecules
    assert np.array_equal(r["indptr"], [0, 1, 3, 3, 4]) and np.array_equal(r["indices"], [2, 0, 4, 1]) and np.array_equal(r["data"], [3, 1, 1, 1])
    assert np.array_equal(r["raw_mapped_reads"], [22]) and np.array_equal(r["flt_mapped_reads"], [0])
    r = N.run(MOL, [0.0, 0.0], CELLS, COLUMNS, 5, FCLASS, 2, CELL_MASK)
    assert np.array_equal(r["indptr"], [0, 0, 0, 0, 0]) and len(r["indices"]) == 0 and not r["raw_mapped_reads"].any() and not r["kept"].any()
    for bad in ([1.5, 0.0], [-0.1, 1.0], [float("nan"), 1.0]):
        with pytest.raises(ValueError):
            N.run(MOL, bad, CELLS, COLUMNS, 5)


# ---- select_features on a 4 x 3 matrix -------------------------------------------------------------------------------------------------
#            col 0  col 1  col 2
#   row 0      5      .      3
#   row 1      .      7      .
#   row 2      1      .      .
#   row 3      2      .      4
M43 = (np.array([0, 3, 4, 6]), np.array([0, 2, 3, 1, 0, 3]), np.array([5, 1, 2, 7, 3, 4]))


def test_select_features_renumbers_and_keeps_an_emptied_column():
    indptr, indices, data = N.select_features(*M43, [1, 0, 1, 1])            # row 1 leaves: column 1 empties but stays
    assert np.array_equal(indptr, [0, 3, 3, 5]) and np.array_equal(indices, [0, 1, 2, 0, 2]) and np.array_equal(data, [5, 1, 2, 3, 4])
    indptr, indices, data = N.select_features(*M43, [0, 1, 0, 1])
    assert np.array_equal(indptr, [0, 1, 2, 3]) and np.array_equal(indices, [1, 0, 1]) and np.array_equal(data, [2, 7, 4])
    same = N.select_features(*M43, [1, 1, 1, 1])
    assert all(np.array_equal(a, b) for a, b in zip(same, M43))
    indptr, indices, data = N.select_features(*M43, [0, 0, 0, 0])
    assert np.array_equal(indptr, [0, 0, 0, 0]) and len(indices) == 0 and len(data) == 0
    with pytest.raises(IndexError):
        N.select_features(*M43, [1, 1, 1])                                   # row 3 is present


def test_select_barcodes_then_features_is_the_filtered_matrix():
    sub = N.select_barcodes(*M43, [2, 0])
    assert np.array_equal(sub[0], [0, 2, 5]) and np.array_equal(sub[1], [0, 3, 0, 2, 3]) and np.array_equal(sub[2], [3, 4, 5, 1, 2])
    indptr, indices, data = N.select_features(*sub, [1, 0, 0, 1])
    assert np.array_equal(indptr, [0, 2, 4]) and np.array_equal(indices, [0, 1, 0, 1]) and np.array_equal(data, [3, 4, 5, 2])
