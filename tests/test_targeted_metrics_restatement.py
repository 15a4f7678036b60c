"""The restatement tests/targeted_metrics_numpy.py against tests/golden/targeted_metrics_reference.npz (no GPU, no library).

The golden file was recorded once on a CPU with the reference's own Python (lib/python/cellranger/targeted/gmm.py through
scikit-learn): fit_enrichments(..., BOTH_TIED) on three fixtures (50 + 80, 120 + 200 and 180 + 420 genes) and on one input per
guard.  The reference's stage module (calculate_targeted_metrics/__init__.py) and pandas_utils import h5py, which the image does
not have: for the statistics the SAME pandas calls (mean_per_gene_rpu_metrics is a literal copy) were recorded on hand-sized
frames, and the tallies are pinned by hand-computed cases, as tests/subsample_numpy.py does.  Only arrays are in the file.

Compared for equality: the threshold, the class counts, the winner, the iteration counts, every integer.  The fit's floats are held
within `fit_bound` = 16 x the largest relative movement of the restatement's parameters and per-start likelihoods over 8 seeded
permutations of each fixture's genes (measured while recording: 1.6e-14, bound 2.6e-13).  Every fixture runs all 5152 starts and
finds its winner itself: no start and no gene is left out (about 10 s per fixture)."""
import math
import os

import numpy as np
import pytest

import targeted_metrics_numpy as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "targeted_metrics_reference.npz")


@pytest.fixture(scope="module")
def g():
    return dict(np.load(GOLDEN))


def test_the_fixtures_meet_the_conditions(g):
    assert float(g["fit_bound"]) == 16 * float(g["fit_movement"]) and 0 < float(g["fit_movement"]) < 1e-12
    for name in "abc":
        gap, post_margin, stop_margin = g[name + "_conditions"]
        assert gap >= 1e-8 and post_margin >= 1e-6 and stop_margin >= 1e-9, name
        lks = np.sort(g[name + "_restate_lks"])[::-1]
        assert lks[0] - lks[1] == gap and len(lks) == R.N_STARTS == 5152
        assert g[name + "_restate_its"].min() >= 2 and g[name + "_restate_its"].max() < 100      # no start ran into the iteration limit


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_fit_against_the_reference(name, g):
    lab, vals = g[name + "_labels"].astype(bool), g[name + "_values"]
    f = R.fit_enrichments(lab, vals)
    p, cs, bound = g[name + "_ref_params"], g[name + "_ref_class"], float(g["fit_bound"])
    assert f["fitted"] and f["winner"] == int(g[name + "_winner"])
    assert f["log_rpu_threshold"] == p[0] and [f[k] for k in R.CLASS_KEYS] == list(cs)
    assert np.array_equal((vals >= f["log_rpu_threshold"]).astype(np.uint8), g[name + "_enriched"])
    for k, v in zip(R.FIT_KEYS[1:], p[1:]):
        assert abs(f[k] - v) <= bound * abs(v), (k, f[k], v)
    assert f["sd_high"] == f["sd_low"]      # the reference reports the tied precision twice
    assert len(f["its"]) == len(f["lks"]) == R.N_STARTS
    assert np.array_equal(f["its"], g[name + "_restate_its"])
    assert np.array_equal(f["lks"], g[name + "_restate_lks"])      # the same code on the same machine type: bit for bit
    assert f["max_lk"] == float(g[name + "_restate_max_lk"])


@pytest.mark.parametrize("guard", ["empty", "no_offtarget", "too_few", "no_targeted"])
def test_guards_against_the_reference(guard, g):
    f = R.fit_enrichments(g["guard_%s_labels" % guard], g["guard_%s_values" % guard])
    assert not f["fitted"]
    assert np.array_equal(np.array([f[k] for k in R.FIT_KEYS]), g["guard_%s_ref_params" % guard], equal_nan=True)
    assert np.array_equal(np.array([f[k] for k in R.CLASS_KEYS]), g["guard_%s_ref_class" % guard], equal_nan=True)


def test_initial_values():
    lab = np.array([1] * 3 + [0] * 4, bool)
    vals = np.array([0.5, 0.1, 0.3, 0.2, 0.8, 0.4, 0.6])
    iw, pairs, prec = R.initial_values(lab, vals)
    assert iw == [3 / 7.0, 4 / 7.0] and list(pairs[0]) == [0.3, 0.5] and len(pairs) == 5152
    assert list(pairs[1]) == [0.0, 0.0] and list(pairs[2]) == [pairs[2][0], 0.0] and list(pairs[-1]) == [0.8, 0.8]
    assert prec == 1.0 / (((0.65 - 0.35) / 1.35) ** 2)


def test_statistics_against_the_recorded_pandas_calls(g):
    names = [str(k) for k in g["stats_names"]]
    for i in range(int(g["n_stats_cases"])):
        c = {k: g["stats%d_%s" % (i, k)] for k in ("num_umis", "num_reads", "num_umis_cells", "num_reads_cells", "is_targeted", "is_gex")}
        st, _ = R.rpu_stats(**c)
        assert np.array_equal(np.array([float(st[k]) for k in names]), g["stats%d_expect" % i], equal_nan=True), i
    # the first hand case by hand: on-target in cells 31/10, 40/25, 40/12
    st, _ = R.rpu_stats(**{k: g["stats0_" + k] for k in ("num_umis", "num_reads", "num_umis_cells", "num_reads_cells", "is_targeted", "is_gex")})
    x = np.sort(np.array([31 / 10, 40 / 25, 40 / 12]))
    assert st["median_reads_per_umi_per_gene_cells_on_target"] == x[1] and st["mean_reads_per_umi_per_gene_cells_on_target"] == x.sum() / 3
    assert st["num_genes_on_target"] == 4 and st["num_genes_quantifiable_off_target"] == 2 and list(st["q_feature"]) == [0, 1, 2, 5, 7]
    assert st["multi_cdna_pcr_dupe_reads_frac_on_target"] == (145 - 62) / 145


def test_tallies_of_the_hand_case():
    mol, cells, nf, expect = R.hand_molecules()
    for libs, exp in expect.items():
        got = R.tallies(mol, nf, libs, cells)
        assert [list(map(int, a)) for a in got] == list(exp), libs
    assert not any(a.any() for a in R.tallies(mol, nf, (0, 1), np.zeros(0, np.uint32))[2:])


def test_summary_of_the_recorded_well(g):
    """the stage's dict from the recorded tallies, with the reference's fit of fixture `a` handed in"""
    med_u, med_g, num_cells, total_reads, frac_on, frac_off = g["e2e_args"]
    fe = dict(zip(R.FIT_KEYS, g["a_restate_params"]))
    fe.update(zip(R.CLASS_KEYS, g["a_ref_class"]))
    s, col = R.targeted_metrics(g["e2e_num_umis"], g["e2e_num_reads"], g["e2e_num_umis_cells"], g["e2e_num_reads_cells"], g["e2e_is_targeted"],
                                g["e2e_is_gex"], med_u, med_g, int(num_cells), int(total_reads), float(frac_on), float(frac_off), fe=fe)
    assert sorted(s) == [str(k) for k in g["e2e_keys"]] and len(s) == 49
    assert np.array_equal(np.array([float(s[k]) for k in sorted(s)]), g["e2e_values"], equal_nan=True)
    assert np.array_equal(col, g["e2e_enriched_rpu"], equal_nan=True)
    assert s["frac_on_target_genes_enriched"] == 34 / 50 and s["num_genes_quantifiable_on_target"] == 50 and math.isclose(s["log_rpu_threshold"], 0.4184155943818352)
