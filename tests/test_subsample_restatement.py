"""The numpy restatement of the read subsampling (tests/subsample_numpy.py) against hand-computed cases, its draw against the
binomial it replaces, and the C host functions crgpu_subsample_plan / crgpu_subsample_summary against the restatement (exact
f64 equality).  No GPU: the library loads without one."""
import numpy as np
import pytest

import subsample_numpy as R


@pytest.fixture(scope="module", autouse=True)
def built_library():
    from cellranger_amd import build

    build.build()


# ---- hand-computed tallies --------------------------------------------------------------------------------------------------------
# 3 barcodes (ranks 10, 20, 30), 4 features (0, 1: genome 0; 2, 3: genome 1), 2 libraries.  Cells: 10 (of both genomes) and 30 (of
# genome 0 only); 20 is no cell.  Feature 0 of barcode 10 is present in both libraries.
BC = np.array([10, 10, 10, 10, 20, 20, 30, 30, 30])
LIB = np.array([0, 1, 0, 0, 0, 1, 0, 0, 1])
FEAT = np.array([0, 0, 1, 2, 0, 3, 1, 2, 2])
KEPT = np.array([2, 1, 0, 3, 1, 2, 4, 5, 0])
FG = np.array([0, 0, 1, 1])
CELLS = np.array([10, 30])
CGM = np.array([3, 1])
EXPECTED = {
    R.PER_CELL: dict(upb=[[2, 1], [1, 0]], rpb=[[3, 4], [3, 0]], fpb=[[1, 1], [1, 0]], rp=[8, 10], um=[4, 3],
                     tfd=[[2, 1, 0, 0], [0, 0, 1, 0]]),
    R.CELLS_ONLY: dict(upb=[[2, 1], [1, 0]], rpb=[[3, 4], [3, 0]], fpb=[[1, 1], [1, 0]], rp=[7, 3], um=[3, 1],
                       tfd=[[2, 1, 0, 0], [0, 0, 1, 0]]),
    R.BULK: dict(upb=[[4, 4], [3, 3]], rpb=[[8, 8], [10, 10]], fpb=[[0, 0], [0, 0]], rp=[8, 10], um=[4, 3],
                 tfd=[[3, 1, 0, 0], [0, 0, 2, 1]]),
}


@pytest.mark.parametrize("task_type", [R.PER_CELL, R.CELLS_ONLY, R.BULK])
def test_hand_computed_tallies(task_type):
    got = R.run_task(task_type, [0.5, 0.5], BC, LIB, FEAT, KEPT, CELLS, CGM, FG, 2, 4)
    e = EXPECTED[task_type]
    for g, k in zip(got, ("upb", "rpb", "fpb", "rp", "um", "tfd")):
        assert np.array_equal(g, np.array(e[k])), k


@pytest.mark.parametrize("rates", [[0.0, 0.0], [np.nan, 0.5], [0.5, np.nan]])
def test_all_zero_and_nan_rates_give_zeros(rates):
    for task_type in (R.PER_CELL, R.CELLS_ONLY, R.BULK):
        got = R.run_task(task_type, rates, BC, LIB, FEAT, KEPT, CELLS, CGM, FG, 2, 4)
        assert all(not g.any() for g in got)


def test_nan_rate_of_an_absent_library_does_not_stop_the_task():
    only0 = LIB == 0
    got = R.run_task(R.PER_CELL, [0.5, np.nan], BC[only0], LIB[only0], FEAT[only0], KEPT[only0], CELLS, CGM, FG, 2, 4)
    assert got[3].tolist() == [7, 8] and got[4].tolist() == [3, 2]
    with pytest.raises(ValueError):
        R.run_task(R.PER_CELL, [1.5, 0.5], BC, LIB, FEAT, KEPT, CELLS, CGM, FG, 2, 4)


def test_run_uses_table_positions_before_the_feature_mask():
    mol = dict(bc=BC, lib=LIB, feature=FEAT, read_count=np.array([5, 3, 2, 7, 1, 4, 6, 9, 2]))
    mask = np.array([0, 1, 1, 1])
    got = R.run([R.PER_CELL], [[0.5, 0.5]], mol, CELLS, 2, FG, CGM, feature_mask=mask, seed=7)
    k = R.kept(mol["read_count"], LIB, [0.5, 0.5], seed=7)          # every molecule keeps the stream of its table position
    keep = mask[FEAT].astype(bool)
    want = R.run_task(R.PER_CELL, [0.5, 0.5], BC[keep], LIB[keep], FEAT[keep], k[keep], CELLS, CGM, FG, 2, 4)
    assert np.array_equal(got["read_pairs"][0], want[3]) and np.array_equal(got["umis_per_bc"][0], want[0])
    assert got["any_reads"].tolist() == [[True, True], [False, True]]  # feature 0 is masked out: library 1 has genome 1 only


# ---- the draw ---------------------------------------------------------------------------------------------------------------------
def _bounds(n_mol, count, rate):
    """exact mean and 5 standard deviations of sum(kept) and of #{kept == 0} for kept ~ Binomial(count, T / 2^53)"""
    p = R.thresholds([rate])[0] / 2.0 ** 53
    q0 = (1.0 - p) ** count
    return (n_mol * count * p, 5.0 * np.sqrt(n_mol * count * p * (1.0 - p))), (n_mol * q0, 5.0 * np.sqrt(n_mol * q0 * (1.0 - q0)))


@pytest.mark.parametrize("n_mol,count,rate", [(20000, 4, 0.3), (2000, 300, 0.05)])
def test_draw_is_the_binomial(n_mol, count, rate):
    counts, libs = np.full(n_mol, count), np.zeros(n_mol, np.int64)
    (m_sum, d_sum), (m_zero, d_zero) = _bounds(n_mol, count, rate)
    for name, k in (("philox", R.kept(counts, libs, [rate], seed=1)), ("numpy", np.random.RandomState(1).binomial(counts, rate))):
        print(name, int(k.sum()), m_sum, d_sum, int((k == 0).sum()), m_zero, d_zero)
        assert abs(k.sum() - m_sum) <= d_sum, name
        assert abs((k == 0).sum() - m_zero) <= d_zero, name
        assert k.min() >= 0 and k.max() <= count


def test_draw_endpoints_and_nesting():
    counts = np.array([1, 3, 4, 5, 8, 70, 300])
    libs = np.zeros(len(counts), np.int64)
    assert np.array_equal(R.kept(counts, libs, [1.0]), counts)
    assert not R.kept(counts, libs, [0.0]).any()
    k = R.kept_all_tasks(counts, libs, [[0.01], [0.5], [0.9]])
    assert np.all(k[0] <= k[1]) and np.all(k[1] <= k[2])            # one set of words: nested in the rate
    assert np.array_equal(k[1], R.kept(counts, libs, [0.5]))
    w = R.read_words(3, 9, seed=1)                                    # word j = word j & 3 of block 1 + (j >> 2) of stream 3
    raw = np.random.Philox(counter=[0, 3, 0, 0], key=[1, 0]).random_raw(12)
    assert np.array_equal(w, raw[:9] >> np.uint64(11))


def test_vectorised_draw_equals_the_loop():
    counts = np.array([1, 3, 4, 5, 8, 0, 70, 300, 2, 9])
    libs = np.array([0, 1, 0, 1, 0, 1, 0, 1, 1, 0])
    pos = np.array([0, 1, 2, 3, 40, 5, 6, 7, 2 ** 31 + 5, 9])
    for rates in ([0.3, 0.9], [1.0, 0.0]):
        assert np.array_equal(R.kept_vectorised(counts, libs, rates, seed=5, positions=pos), R.kept(counts, libs, rates, seed=5, positions=pos))
    assert np.array_equal(R.kept_vectorised(counts, libs, [0.5, 0.5]), R.kept(counts, libs, [0.5, 0.5]))


# ---- the plan ---------------------------------------------------------------------------------------------------------------------
PLAN_CASE = dict(lib_indices=[0, 1], num_cells_per_lib=[100, 100], raw_reads_per_lib=[1_000_000, 2_000_000],
                 usable_reads_per_lib=[500_050, 1_500_000])


def test_plan_hand_computed():
    """MAPPED: usable reads per cell = [5000.5, 15000] -> max 5000.5, step 500.05: 500, 1000, ..., 4500 and trunc(5000.5) = 5000"""
    depths, rates = R.plan(R.PLAN_MAPPED, fixed_depths=[3000, 20000], **PLAN_CASE)
    assert depths.tolist() == [500, 1000, 1500, 2000, 2500, 3000, 3500, 4000, 4500, 5000, 20000]
    assert rates.shape == (11, 2)
    assert rates[0].tolist() == [500 * 100.0 / 500_050, 500 * 100.0 / 1_500_000]
    r0, r1 = 5000 * 100.0 / 500_050, 5000 * 100.0 / 1_500_000             # the largest computed depth: renormalised
    assert r0 < 1.0 and rates[9].tolist() == [r0 / r0, r1 / r0] and rates[9, 0] == 1.0
    assert rates[10].tolist() == [0.0, 0.0]                               # 20000: both rates exceed 1
    depths, rates = R.plan(R.PLAN_RAW, fixed_depths=[20000], **PLAN_CASE)  # raw reads per cell = [10000, 20000]
    assert depths.tolist() == [1000 * i for i in range(1, 11)] + [20000]
    f0, f1 = 500_050 / 1_000_000, 1_500_000 / 2_000_000
    assert rates[2].tolist() == [3000 * 100.0 * f0 / 500_050, 3000 * 100.0 * f1 / 1_500_000]
    assert rates[10, 0] == 0.0 and rates[10, 1] == 20000 * 100.0 * f1 / 1_500_000
    depths, rates = R.plan(R.PLAN_BULK, fixed_depths=[10_000, 5_000_000], **PLAN_CASE)
    assert depths.tolist() == [10_000] + [100_000 * i for i in range(1, 11)] + [5_000_000]
    assert rates[depths.tolist().index(1_000_000)].tolist() == [1.0, 0.5]
    assert rates[-1].tolist() == [0.0, 0.0]


def test_plan_of_one_library_leaves_the_others_at_zero():
    depths, rates = R.plan(R.PLAN_MAPPED, [1], [100, 100], [1e6, 2e6], [5e5, 1.5e6], [3000])
    assert np.all(rates[:, 0] == 0.0) and rates[-1, 1] == 1.0 and depths[-1] == 15000


def test_compute_target_depths_edges():
    assert R.compute_target_depths(0.7, 10).tolist() == []
    assert R.compute_target_depths(4.0, 10).tolist() == [1, 2, 3, 4]          # max < num: fewer targets
    assert R.compute_target_depths(3.9, 10).tolist() == [1, 2, 3]
    assert R.compute_target_depths(10.0, 10).tolist() == list(range(1, 11))


# ---- the summary ------------------------------------------------------------------------------------------------------------------
def _summary_data():
    # task 0: per cell, 4 cells of genome 0 (even), 3 of genome 1 (odd); task 1: bulk; task 2: no reads at all
    upb = np.array([[[5, 1, 9, 2], [4, 0, 7, 3]], [[17, 17, 17, 17], [14, 14, 14, 14]], [[0] * 4, [0] * 4]], np.int64)
    rpb = upb * 3 + 1
    rpb[2] = 0
    fpb = np.array([[[3, 1, 4, 2], [2, 0, 5, 1]], [[0] * 4, [0] * 4], [[0] * 4, [0] * 4]], np.int64)
    rp = np.array([[60, 50], [55, 45], [0, 0]], np.int64)
    um = np.array([[17, 14], [17, 14], [0, 0]], np.int64)
    tfd = np.zeros((3, 2, 6), np.int64)
    tfd[1, 0, [0, 2, 5]] = [4, 1, 12]
    tfd[1, 1, 3] = 14
    return dict(umis_per_bc=upb, read_pairs_per_bc=rpb, features_det_per_bc=fpb, read_pairs=rp, umis=um, total_features_det=tfd)


SUMMARY_TYPES = [R.PER_CELL, R.BULK, R.PER_CELL]
SUMMARY_CGM = np.array([3, 1, 3, 3])   # cell 1 is no cell of genome 1


def test_summary_hand_computed():
    out, allf = R.summary(_summary_data(), SUMMARY_TYPES, SUMMARY_CGM)
    assert out[0, 0].tolist() == [13.75, 11.5, 4.25, 3.5, 2.5, 2.5, 43 / 60]       # even: the mean of the two middle values
    assert out[0, 1].tolist() == [15.0, 13.0, 14 / 3, 4.0, 8 / 3, 2.0, 36 / 50]   # odd (cells 0, 2, 3)
    assert out[1, 0, 4:6].tolist() == [3.0, 3.0] and out[1, 1, 4:6].tolist() == [1.0, 1.0]
    assert out[2, 0].tolist() == [0.0] * 7 and allf.tolist() == [79 / 110, 69 / 100, 0.0]
    out, _ = R.summary(_summary_data(), SUMMARY_TYPES, np.array([1, 1, 1, 1]))       # no cell of genome 1: NaN, as numpy
    assert np.isnan(out[0, 1, :6]).all() and out[0, 1, 6] == 36 / 50


# ---- the C host functions == the restatement ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("stype", [R.PLAN_RAW, R.PLAN_MAPPED, R.PLAN_RAW_CELLS, R.PLAN_BULK])
@pytest.mark.parametrize("case", ["two_libs", "one_of_two", "tiny", "below_one", "zero_usable"])
def test_c_plan_equals_the_restatement(stype, case):
    from cellranger_amd import engine as E

    fixed = R.BULK_FIXED_DEPTHS if stype == R.PLAN_BULK else R.FIXED_DEPTHS
    args = {"two_libs": PLAN_CASE,
            "one_of_two": dict(lib_indices=[1], num_cells_per_lib=[100, 250], raw_reads_per_lib=[1e6, 7_654_321], usable_reads_per_lib=[5e5, 3_333_333]),
            "tiny": dict(lib_indices=[0], num_cells_per_lib=[1000], raw_reads_per_lib=[4100], usable_reads_per_lib=[3900]),
            "below_one": dict(lib_indices=[0], num_cells_per_lib=[1000], raw_reads_per_lib=[700], usable_reads_per_lib=[600]),
            "zero_usable": dict(lib_indices=[0, 1], num_cells_per_lib=[50, 50], raw_reads_per_lib=[1e5, 2e5], usable_reads_per_lib=[0, 1e5])}[case]
    if stype == R.PLAN_BULK and case in ("tiny", "below_one"):
        fixed = [100, 1000]
    want_d, want_r = R.plan(stype, fixed_depths=fixed, **args)
    got_d, got_r = E.subsample_plan(stype, fixed_depths=fixed, **args)
    assert np.array_equal(got_d, want_d)
    assert got_r.shape == want_r.shape and np.array_equal(got_r, want_r, equal_nan=True)


def test_c_plan_defaults_sizes_and_refusals():
    from cellranger_amd import _lib
    from cellranger_amd import engine as E

    d, r = E.subsample_plan(_lib.SS_PLAN_MAPPED, **PLAN_CASE)
    assert np.array_equal(d, R.plan(R.PLAN_MAPPED, fixed_depths=R.FIXED_DEPTHS, **PLAN_CASE)[0])
    assert (list(_lib.SS_FIXED_DEPTHS), list(_lib.SS_TARGETED_FIXED_DEPTHS), list(_lib.SS_BULK_FIXED_DEPTHS)) == \
        (R.FIXED_DEPTHS, R.TARGETED_FIXED_DEPTHS, R.BULK_FIXED_DEPTHS)
    with pytest.raises(E.CrgpuError) as e:                       # no cells: the feasible depth is infinite
        E.subsample_plan(_lib.SS_PLAN_RAW, [0], [0], [1e6], [5e5])
    assert e.value.code == -1
    with pytest.raises(E.CrgpuError):
        E.subsample_plan(_lib.SS_PLAN_RAW, [2], [10, 10], [1e6, 1e6], [5e5, 5e5])


@pytest.mark.parametrize("cgm", [None, SUMMARY_CGM, np.array([1, 1, 1, 1])])
def test_c_summary_equals_the_restatement(cgm):
    from cellranger_amd import engine as E

    want, want_all = R.summary(_summary_data(), SUMMARY_TYPES, cgm)
    got, got_all = E.subsample_summary(_summary_data(), SUMMARY_TYPES, cgm)
    assert np.array_equal(got, want, equal_nan=True) and np.array_equal(got_all, want_all)
