"""The numpy restatement tests/aggregates_numpy.py against the reference's own outputs, recorded by scripts/make_aggregates_golden.py in
tests/golden/aggregates_reference.npz (no GPU).  The recorded fixtures are tie-insensitive, so both tie rules must reproduce them.
reads_removed / reads_total is ONE division where the reference sums n per-barcode quotients reads_i / total: each quotient is rounded
once (relative 2^-53), each of the n - 1 additions of positive terms rounds once more (relative 2^-53 of a partial sum that is at most
the result), and the single division rounds once: (2 n + 2) * 2^-53 relative covers the difference.
The closing filters' reference module cannot be imported outside the pipeline (tests/aggregates_numpy.py says why): hand cases."""
import os

import numpy as np
import pytest

import aggregates_numpy as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "aggregates_reference.npz")
FIXTURES = R.golden_fixtures()


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def test_fraction_to_use_is_the_recorded_one(golden):
    assert list(golden["fraction_n"]) == list(range(5, 65))
    for n, f in zip(golden["fraction_n"], golden["fraction"]):
        assert R.fraction_to_use(int(n)) == f
    # by hand: 5 * 1.0, 12 * 0.86 = 10.32, 13 * 0.84 = 10.92, 25 * 0.6, 26 * 0.58 = 15.08, 27 * 0.6 = 16.2
    assert [R.min_antibodies(n) for n in (5, 12, 13, 25, 26, 27)] == [5, 10, 11, 15, 15, 16]


@pytest.mark.parametrize("tie", ["high", "low"])
@pytest.mark.parametrize("name", [n for n, _ in FIXTURES])
def test_restatement_equals_the_recorded_reference(golden, name, tie):
    fx = dict(FIXTURES)[name]
    got = R.remove_aggregates(fx, tie)
    for key, bit in (("aggregates", R.COUNTS), ("outliers", R.ANTIGEN), ("highly_corrected", R.HIGHLY_CORRECTED)):
        assert np.array_equal(got["removed"][(got["reasons"] & bit) != 0], golden[name + "/" + key]), key
    assert np.array_equal(np.union1d(got["removed"], got["kept"]), np.arange(len(fx["indptr"]) - 1, dtype=np.uint64))


def test_the_fixtures_cover_both_outcomes_and_both_probe_counts(golden):
    n_agg = [len(golden[n + "/aggregates"]) for n, _ in FIXTURES]
    assert sum(k > 0 for k in n_agg) >= 4 and 0 in n_agg
    assert any(len(golden[n + "/outliers"]) for n, _ in FIXTURES)
    assert {fx["num_probe_barcodes"] for _, fx in FIXTURES} == {None, 1, 2}
    assert {R.remove_aggregates(fx)["info"]["n_signal"] < 5 for _, fx in FIXTURES} == {True, False}


@pytest.mark.parametrize("name", [n for n, _ in FIXTURES])
def test_one_division_against_the_reference_sum_of_quotients(golden, name):
    got = R.remove_aggregates(dict(FIXTURES)[name])
    for lib, ref in zip((R.AB, R.AG), golden[name + "/reads_lost"]):
        d = got["libraries"][lib]
        n, ours = d["number_aggregate_GEMs"], d["reads_removed"] / d["reads_total"]
        print(name, lib, n, ours, float(ref))
        assert abs(ours - ref) <= (2 * n + 2) * 2.0 ** -53 * abs(ref)


# ---- the closing filters, by hand ---------------------------------------------------------------------------------------------------
def test_minimum_umis_by_hand():
    umis = np.array([0, 5, 9, 10, 11, 3, 10], np.uint32)
    cols = np.array([0, 2, 3, 4, 6], np.uint64)
    assert list(R.apply_minimum_umis(cols, umis, 10)) == [3, 4, 6]
    assert list(R.apply_minimum_umis(cols, umis, 0)) == [0, 2, 3, 4, 6]      # minimum_umis 0 keeps a cell without a count
    assert list(R.apply_minimum_umis(cols, umis, 12)) == []


def test_mito_threshold_by_hand():
    total = np.array([0, 200, 200, 8, 1000, 3], np.uint32)
    mito = np.array([0, 20, 21, 1, 100, 3], np.uint32)
    cols = np.arange(6, dtype=np.uint64)
    kept, removed, tot, pct = R.apply_mito_threshold(cols, mito, total, 10.0)
    # 0 / 0 is NaN and stays; 20 / 200 and 100 / 1000 are exactly 10.0 and stay (>); 21 / 200 = 10.5, 1 / 8 = 12.5 and 3 / 3 leave
    assert list(kept) == [0, 1, 4] and list(removed) == [2, 3, 5]
    assert list(tot) == [200, 8, 3] and list(pct) == [10.5, 12.5, 100.0]
    assert list(R.apply_mito_threshold(cols, mito, total, 100.0)[1]) == []
    assert list(R.apply_mito_threshold(cols, mito, total, -1.0)[0]) == [0]      # only the NaN stays
