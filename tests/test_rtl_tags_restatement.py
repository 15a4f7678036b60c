"""Hand-computed cases that pin tests/rtl_tags_numpy.py, the restatement of CALL_TAGS_RTL and of the high-occupancy-GEM removal
that the device code is compared against (no GPU).  Every expected number below was worked out on paper."""
import math

import numpy as np
import pytest

import rtl_tags_numpy as R

IDS3 = ["BC001", "BC002", "BC003"]
# five GEMs, three probe barcodes; every column is a cell
W5 = [(0, 0), (0, 1), (1, 0), (2, 1), (2, 2), (3, 0), (3, 1), (3, 2), (4, 0)]


def test_three_tags_five_gems_every_overlap_by_hand():
    groups = R.group(W5, IDS3)
    assert {i: sorted(g) for i, g in groups.items()} == {"BC001": [0, 1, 3, 4], "BC002": [0, 2, 3], "BC003": [2, 3]}
    assert R.overlap_rows(groups) == [("BC001", "BC002", 4, 3, 2, 2 / 3), ("BC001", "BC003", 4, 2, 1, 1 / 2), ("BC002", "BC003", 3, 2, 2, 1.0)]
    counts = [{0: 1}] * len(W5)
    per_tag, rows, metrics, umi = R.call_tags_rtl(W5, counts, ["Gene Expression"], IDS3, list(range(len(W5))))
    assert {i: len(v) for i, v in per_tag.items()} == {"BC001": 4, "BC002": 3, "BC003": 2}
    assert metrics["filtered_gel_bead_barcodes_count"] == 5
    assert metrics["filtered_barcodes_per_probe_barcode"] == {"BC001": 4, "BC002": 3, "BC003": 2}
    assert metrics["probe_barcode_overlap_coefficients"] == {"BC001_BC002": 2 / 3, "BC001_BC003": 0.5, "BC002_BC003": 1.0}
    assert umi == {"Gene Expression": {"BC001": 4, "BC002": 3, "BC003": 2}}


def test_two_probe_ranks_of_one_tag_in_one_gem_count_the_gem_once():
    groups = R.group([(7, 0), (7, 1), (8, 2)], ["BC001", "BC001", "BC002"])
    assert groups == {"BC001": {7: 2}, "BC002": {8: 1}}
    assert R.overlap_rows(groups) == [("BC001", "BC002", 1, 1, 0, 0.0)]


def test_a_key_without_entries_gives_a_nan_row():
    rows = R.overlap_rows({"AB001": {}, "BC001": {3: 1}})
    assert rows[0][:5] == ("AB001", "BC001", 0, 1, 0) and math.isnan(rows[0][5])


def test_medians_of_zero_to_three_values():
    assert R.median_of_sorted([]) is None
    assert R.median_of_sorted([5]) == 5
    assert R.median_of_sorted([3, 6]) == 4          # (3 + 6) / 2 in integers
    assert R.median_of_sorted([1, 2, 9]) == 2
    cols = [(0, 0), (0, 1), (1, 0), (1, 1), (2, 0)]
    counts = [{0: 3, 1: 2}, {1: 9}, {0: 6}, {0: 4, 1: 0}, {0: 50}]
    med = R.median_umi_per_cell(cols, counts, ["G", "A"], [0, 1, 2, 3])      # column 4 is no cell
    assert med == {("G", 0): 4, ("A", 0): 2, ("A", 1): 9, ("G", 1): 4}


def test_rust_round_of_a_tenth_of_the_median():
    assert [int(R.rust_round(0.1 * float(m))) for m in (4, 5, 15, 25)] == [0, 1, 2, 3]
    assert R.rust_round(2.5) == 3 and R.rust_round(0.5) == 1 and R.rust_round(1.4999) == 1


def test_categories():
    assert [R.categorize(i) for i in ("BC001", "BC024", "BC025", "AB005", "CR001", "OH001", "BC01A", "CMO301")] == [
        "RTL", "RTL", "Antibody", "Antibody", "Crispr", "Overhang", "RTL", "CMO"]


# two probe ranks; each RTL barcode is paired with an antibody barcode.  Features: 0 = Gene Expression, 1 = Antibody Capture
AB_COLS = [(0, 0), (0, 1), (1, 0), (1, 1), (2, 0), (2, 1)]
AB_COUNTS = [{0: 5, 1: 40}, {0: 3, 1: 100}, {1: 3}, {1: 10}, {0: 7, 1: 20}, {1: 2}]
AB_CELLS = [0, 1, 4]
AB_TYPES = ["Gene Expression", R.ANTIBODY]
AB_IDS = ["BC001", "BC002"]
AB_PAIRS = {"BC001": "AB001", "BC002": "AB002"}


def test_rtl_ab_filter_with_configured_pairings_and_swaps():
    med = R.median_umi_per_cell(AB_COLS, AB_COUNTS, AB_TYPES, AB_CELLS)
    assert med[(R.ANTIBODY, 0)] == 30 and med[(R.ANTIBODY, 1)] == 100          # thresholds 3 and 10
    gex = R.group([AB_COLS[c] for c in AB_CELLS], AB_IDS)
    assert gex == {"BC001": {0: 1, 2: 1}, "BC002": {0: 1}}
    # AB001: GEMs 0 (40), 1 (3), 2 (20) all reach 3; AB002: GEMs 0 (100) and 1 (10) reach 10, GEM 2 (2) does not
    rows = R.suspicious_pairings(AB_COLS, AB_COUNTS, AB_TYPES, AB_IDS, AB_PAIRS, med, gex)
    assert rows == [("BC001", "AB002", 2, 2, 1, 0.5), ("BC002", "AB001", 1, 3, 1, 1.0)]
    # with BC002 unpaired its Antibody counts stay under an RTL identifier with a median: the reference's assert_eq fires
    with pytest.raises(AssertionError):
        R.suspicious_pairings(AB_COLS, AB_COUNTS, AB_TYPES, AB_IDS, {"BC001": "AB001"}, med, gex)
    all_rows = [("AB001", "BC001", 3, 2, 2, 1.0), ("AB001", "BC002", 3, 1, 1, 1.0), ("AB001", "AB002", 3, 2, 2, 1.0), ("BC001", "BC002", 2, 1, 1, 1.0)]
    assert R.filter_suspicious(all_rows, {"BC001": "AB001"}) == [("BC002", "AB001", 1, 3, 1, 1.0)]
    _, rows, metrics, _ = R.call_tags_rtl(AB_COLS, AB_COUNTS, AB_TYPES, AB_IDS, AB_CELLS, AB_PAIRS)
    assert rows == [("BC001", "BC002", 2, 1, 1, 1.0), ("BC001", "AB002", 2, 2, 1, 0.5), ("BC002", "AB001", 1, 3, 1, 1.0)]
    assert set(metrics["probe_barcode_overlap_coefficients"]) == {"BC001_BC002", "BC001_AB002", "BC002_AB001"}


def test_a_tag_without_a_cell_with_antibody_counts_is_removed():
    counts = [{0: 5}, {0: 3, 1: 100}, {1: 3}, {1: 10}, {0: 7}, {1: 2}]         # no cell of probe 0 holds Antibody counts
    med = R.median_umi_per_cell(AB_COLS, counts, AB_TYPES, AB_CELLS)
    gex = R.group([AB_COLS[c] for c in AB_CELLS], AB_IDS)
    rows = R.suspicious_pairings(AB_COLS, counts, AB_TYPES, AB_IDS, AB_PAIRS, med, gex)
    assert rows == [("BC001", "AB002", 2, 2, 1, 0.5)]


def test_lambda_of_a_hand_histogram():
    hist, lam, probes, per_gem = R.occupancy(W5, partitions=10, recovery_factor=0.5)
    assert hist == {2: 2, 1: 2, 3: 1, 0: 0} and lam == 9 / 5 and probes == 3 and len(per_gem) == 5
    hist, lam, _, _ = R.occupancy(W5)
    assert hist[0] == 69691 and lam == 9 / 69696          # int(115000 * (1 / 1.65) - 5) = int(69691.97)
    assert R.occupancy(W5, partitions=4, recovery_factor=1.0)[0][0] == 0       # never negative


def test_removal_at_threshold_one():
    kept, n_high, n_cells, f_gems, f_cells = R.remove_high_occupancy(W5, 1)
    assert kept == [2, 8] and n_high == 3 and n_cells == 7 and f_gems == 3 / 5 and f_cells == 7 / 9
    assert R.remove_high_occupancy(W5, 3)[:3] == (list(range(9)), 0, 0)
    assert R.remove_high_occupancy(W5, 0)[:3] == ([], 5, 9)
    out = R.remove_high_occupancy([], 1)
    assert out[:3] == ([], 0, 0) and math.isnan(out[3]) and math.isnan(out[4])


def test_threshold_simulation_runs_on_numpys_legacy_stream():
    assert R.threshold(0, ["a"]) == 0
    probes = [p for _, p in W5]
    t = R.threshold(1.8, probes, total_simulated_gems=5000)
    # the same call by hand: what numpy's legacy stream gives
    np.random.seed(0)
    g = np.random.poisson(1.8, 5000)
    g = g[g > 0]
    sim = np.random.choice(3, size=(len(g), g.max()), p=np.array([4, 3, 2]) / 9)
    assert t == int(np.ceil(np.quantile([len(set(sim[i, :k])) for i, k in enumerate(g)], 0.999))) == 3
