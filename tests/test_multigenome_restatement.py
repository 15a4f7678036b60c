"""Pins tests/multigenome_numpy.py (the numpy restatement the device path is compared with) on cases worked out by hand from
the contract of lib/python/cellranger/analysis/multigenome.py:80-335: the percentile's interpolation, the default branch, a
tie cell, the fold-change fallback, the inference's zero class and its cap, the purities, the choice of the two genomes."""
import numpy as np

import multigenome_numpy as R


def _p10(x):
    """the contract's restatement of np.percentile(x, 10.0) on integers"""
    x = sorted(x)
    M = len(x)
    v = (M - 1) * 0.1
    lo = int(np.floor(v))
    g, hi = v - lo, min(lo + 1, M - 1)
    d = x[hi] - x[lo]
    return x[hi] - d * (1 - g) if g >= 0.5 else x[lo] + d * g


def test_percentile_formula_at_small_sizes():
    # M = 1: the value itself; M = 2: v = 0.1 between the two; M = 11: v = 1.0 exactly, the second smallest
    assert np.percentile([7], 10.0) == _p10([7]) == 7.0
    assert np.percentile([10, 20], 10.0) == _p10([10, 20]) == 11.0
    x = [5, 100, 3, 50, 70, 90, 20, 30, 40, 60, 80]
    assert np.percentile(x, 10.0) == _p10(x) == 5.0
    # g >= 0.5: M = 6 gives v = 0.5, M = 8 gives v = 0.7000000000000001: the formula counts back from the upper value
    assert np.percentile([0, 7, 9, 9, 9, 9], 10.0) == _p10([0, 7, 9, 9, 9, 9]) == 7 - 7 * (1 - 0.5) == 3.5
    x8 = [3, 13, 20, 21, 22, 23, 24, 25]
    g = 7 * 0.1 - 0.0
    assert g >= 0.5 and np.percentile(x8, 10.0) == _p10(x8) == 13 - 10 * (1 - g)
    rng = np.random.RandomState(3)
    for _ in range(300):
        x = rng.randint(0, 5000, rng.randint(1, 40)).tolist()
        assert np.percentile(x, 10.0) == _p10(x)


def test_percentile_branch_and_classes():
    # A = {700, 750, 800, 900}: v = 0.3 -> 700 + 50 * 0.3 = 715; B = {600, 500}: v = 0.1 -> 500 + 100 * 0.1 = 510
    c0, c1 = [900, 800, 700, 5, 3, 750], [10, 7, 0, 600, 500, 520]
    call, t0, t1, branch = R.classify(c0, c1)
    assert branch == 1 and t0 == 715.0
    assert t0 == 700 + 50 * 0.30000000000000004 == np.percentile([900, 800, 700, 750], 10.0)
    assert t1 == 510.0
    assert call.tolist() == [0, 0, 0, 1, 1, 2]          # (750, 520) reaches both thresholds


def test_default_branch_when_one_side_is_empty():
    call, t0, t1, branch = R.classify([100, 50, 9], [0, 12, 3])       # no cell with c1 > c0
    assert (t0, t1, branch) == (10.0, 10.0, 0)
    assert call.tolist() == [0, 2, 0]                                  # (50, 12) >= (10, 10); (9, 3) is not
    call, t0, t1, branch = R.classify([0, 0], [0, 0])                  # neither side
    assert branch == 0 and call.tolist() == [0, 0]


def test_a_tie_cell_is_in_neither_percentile_and_is_genome0():
    c0, c1 = [100, 200, 40, 1], [1, 2, 40, 300]
    call, t0, t1, branch = R.classify(c0, c1)
    assert branch == 1 and t0 == 100 + 100 * 0.1 and t1 == 300.0      # the (40, 40) cell does not enter A or B
    assert call.tolist() == [0, 0, 0, 1]
    call, _, _, _ = R.classify([100, 200, 400, 1], [1, 2, 400, 300])  # a tie above both thresholds is a Multiplet
    assert call.tolist() == [0, 0, 2, 1]


def test_fold_change_replaces_both_thresholds_by_the_percentile_of_the_sums():
    # t0 = P10{1000, 1100, 1200} = 1020, t1 = P10{1, 2} = 1.1: lo < 50 and 1020 / 1.1 > 25
    c0, c1 = [1000, 1100, 1200, 0, 1], [0, 1, 0, 1, 2]
    call, t0, t1, branch = R.classify(c0, c1)
    sums = sorted([1000, 1101, 1200, 1, 3])                            # v = 0.4: 1 + 2 * 0.4
    assert branch == 3 and t0 == t1 == sums[0] + (sums[1] - sums[0]) * 0.4 == 1.8
    assert call.tolist() == [0, 0, 0, 1, 1]                            # (1, 2): c0 = 1 < 1.8
    # (a percentile of A or B is at least 1, the smallest count that can exceed another: the ratio never divides by zero)
    # lo >= 50: no fallback whatever the ratio
    _, t0, t1, branch = R.classify([50_000, 60_000, 1], [0, 1, 60])
    assert branch == 1 and (t0, t1) == (51_000.0, 60.0)


def test_infer_with_a_zero_class_and_with_the_cap():
    assert R.infer(5, 0, 7) == 0 and R.infer(5, 7, 0) == 0 and R.infer(0, 0, 0) == 0
    assert R.infer(0, 3, 4) == 0.0
    assert R.infer(1, 5, 5) == 1 / (2 * 0.5 * 0.5) == 2.0
    # m / p beyond all barcodes: 6 / (2 * (1 / 3) * (2 / 3)) = 13.5 > 9
    assert 6 / (2 * (1.0 / 3.0) * (2.0 / 3.0)) > 9 and R.infer(6, 1, 2) == 9.0
    assert R.infer(2, 1, 2) == 2 / (2 * (1.0 / 3.0) * (2.0 / 3.0))     # 4.5 <= 5: not capped


def test_summary_and_purity():
    bc = np.array([[1, 5, 5], [0, 3, 4], [6, 1, 2], [5, 0, 7]])
    s = R.summary(bc, 11)
    assert s["boot"].tolist() == [2.0, 0.0, 9.0, 0.0] and s["mean"] == 2.75 and s["inferred_multiplets"] == 3
    assert s["rate"] == 2.75 / 11 and s["normalized_rate"] == 1000 * (2.75 / 11) / 11
    assert s["rate_lb"] == 0.0 and s["rate_ub"] == np.percentile([0.0, 0.0, 2.0, 9.0], 97.5) / 11
    one = R.summary(bc[:1], 11)
    assert one["rate_lb"] is None and one["rate_ub"] is None and one["inferred_multiplets"] == 2
    assert R.summary(np.array([[1, 5, 5], [2, 2, 2], [1, 5, 5], [1, 5, 5]]), 6)["inferred_multiplets"] == 2     # (2 + 4 + 2 + 2) / 4 = 2.5 rounds to even
    assert R.summary(np.array([[1, 5, 5], [5, 3, 3]]), 11)["inferred_multiplets"] == 6    # (2 + 10) / 2
    sums, pur = R.purity([90, 5, 40, 7], [10, 45, 60, 7], [0, 1, 2, 0])
    assert sums == (97, 114, 45, 50, 142, 164) and pur == (97 / 114, 45 / 50, 142 / 164)
    sums, pur = R.purity([3], [4], [2])
    assert sums == (0,) * 6 and all(np.isnan(p) for p in pur)


def test_top_two_takes_the_larger_index_among_equal_totals():
    assert R.top_two([5, 9, 7]) == [1, 2]
    assert R.top_two([7, 7, 7]) == [1, 2]
    assert R.top_two([9, 4, 4]) == [0, 2]
    assert R.top_two([3, 8]) == [0, 1]


def test_bootstrap_draws_are_the_accepted_words_of_the_raw_stream():
    """np.random.seed(0) + choice(n, n) per sample == RandomState(0)'s 32-bit outputs, masked, rejected above n - 1"""
    n = 1000
    np.random.seed(0)
    got = np.concatenate([np.random.choice(n, n) for _ in range(3)])
    raw = np.random.RandomState(0).randint(0, 1 << 32, 8000, dtype=np.uint64).astype(np.uint32) & np.uint32(1023)
    assert np.array_equal(got, raw[raw <= n - 1][:3000])
    # the fixtures of the GPU tests: branch counts over the 1000 samples
    c0, c1 = [900, 800, 700, 650, 12, 3, 40, 0, 5], [10, 7, 0, 30, 600, 500, 40, 0, 450]
    counts, thr, br = R.bootstrap(c0, c1)
    assert np.bincount(br, minlength=4).tolist() == [25, 975, 0, 0]
    assert int(((counts[:, 1] == 0) | (counts[:, 2] == 0)).sum()) == 21 and (counts.sum(axis=1) == 9).all()
