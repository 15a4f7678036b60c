"""CPU checks that pin tests/emptydrops_numpy.py, the expected side of the EmptyDrops GPU tests, without the library:

* against the reference's own recorded outputs (tests/golden/emptydrops_reference.npz, written by
  scripts/make_emptydrops_golden.py from cellranger.sgt / cellranger.stats): profile, observed log-likelihoods, and the
  p-values and calls of the Philox simulation against those of the reference's np.random simulation;
* its Philox4x64-10 against numpy's."""
import os

import numpy as np
import pytest

import emptydrops_numpy as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "emptydrops_reference.npz")
# Measured once on the fixture: the restatement's profile_p agrees with the recorded one to 2.3e-16 and its gammaln route of
# the observed log-likelihood with the recorded scipy multinomial.logpmf to 2.3e-15 (relative).  Fixed at 100 x that.
RTOL = 2.5e-13


def load_fixture():
    """(golden arrays, CSC of the fixture well, initial cells): make_well(seed) without its three largest cells"""
    g = np.load(GOLDEN)
    indptr, indices, data, nf, kind = R.make_well(int(g["well_seed"]))
    umis = R.column_sums(indptr, indices, data, nf)
    cells = np.flatnonzero(kind == 0)
    cells = np.sort(cells[np.argsort(umis[cells], kind="stable")[:-int(g["dropped_cells"])]])
    return g, (indptr, indices, data, nf), kind, cells


@pytest.fixture(scope="module")
def fixture_run():
    g, csc, kind, cells = load_fixture()
    r = R.find_nonambient(*csc, cells, int(g["low"]), int(g["high"]), int(g["minimum_umis"]), int(g["num_sims"]), float(g["fdr"]), seed=0)
    return g, csc, kind, cells, r


def test_fixture_inputs_are_the_recorded_ones(fixture_run):
    """the well is rebuilt from its seed: what the reference was given must be what the restatement sees"""
    g, (indptr, indices, data, nf), kind, cells, r = fixture_run
    assert r["status"] == R.STATUS_OK
    assert np.array_equal(cells, g["cell_cols"])
    assert r["n_ambient_used"] == int(g["n_ambient_used"]) and r["max_background_umis"] == int(g["max_background_umis"])
    assert np.array_equal(r["eval_features"], g["eval_features"])
    assert np.array_equal(r["eval_cols"], g["eval_cols"]) and np.array_equal(r["umis"], g["umis"])
    for k, c in enumerate(r["eval_cols"]):
        a, b = g["cand_indptr"][k], g["cand_indptr"][k + 1]
        assert np.array_equal(indices[indptr[c]:indptr[c + 1]], g["cand_indices"][a:b])
        assert np.array_equal(data[indptr[c]:indptr[c + 1]], g["cand_data"][a:b])
    step = np.diff(g["ref_sim_n"])      # every branch of the reference's loop (stats.py:143-197) was taken
    assert (step == 1).any() and ((step >= 2) & (step < 20)).any() and ((step >= 20) & (step < 1000)).any() and (step >= 1000).any()
    assert np.array_equal(r["sim_n"], g["ref_sim_n"])


def test_profile_and_observed_loglk_equal_the_references(fixture_run):
    """relative RTOL = 2.5e-13: 100 x the 2.3e-15 measured between the gammaln route and scipy's multinomial.logpmf"""
    g, csc, kind, cells, r = fixture_run
    prof = g["profile"]
    pstar, p0, _ = R.sgt_proportions(prof[prof > 0])
    assert np.all(np.abs(pstar - g["ref_pstar"]) <= RTOL * g["ref_pstar"]) and abs(p0 - float(g["ref_p0"])) <= RTOL * p0
    assert np.all(np.abs(r["profile_p"] - g["ref_profile_p"]) <= RTOL * g["ref_profile_p"])
    assert np.all(np.abs(r["obs_loglk"] - g["ref_obs_loglk"]) <= RTOL * np.abs(g["ref_obs_loglk"]))


def test_philox_simulation_agrees_with_the_references_simulation(fixture_run):
    """two independent simulations of the same null: per candidate the p-values are two binomial proportions, compared at 5
    pooled standard deviations; the calls are equal wherever the reference's adjusted p-value is outside [fdr / 2, 2 fdr],
    and that band holds at most 5 % of the candidates"""
    g, csc, kind, cells, r = fixture_run
    S, fdr = int(g["num_sims"]), float(g["fdr"])
    p, q = r["pvalues"], g["ref_pvalues"]
    pm = (p + q) / 2
    bound = 5 * np.sqrt(2 * np.maximum(pm * (1 - pm), 1.0 / S) / S)
    print("largest |p - p_ref| / bound:", np.max(np.abs(p - q) / bound))
    assert np.all(np.abs(p - q) <= bound)
    adj = g["ref_pvalues_adj"]
    band = (adj >= fdr / 2) & (adj <= 2 * fdr)
    assert band.sum() <= 0.05 * len(adj)
    assert np.array_equal(r["is_nonambient"][~band], (adj <= fdr)[~band])
    k = kind[r["eval_cols"]]
    assert (k == 3).sum() == 60 and r["is_nonambient"][k == 3].all() and np.all(r["pvalues"][k == 3] == 1.0 / (S + 1))
    assert np.all(q[k == 3] == 1.0 / (S + 1))      # ... as in the reference
    assert r["is_nonambient"][k == 2].sum() <= 2
    assert np.array_equal(r["called_cols"], np.union1d(cells, r["eval_cols"][r["is_nonambient"]]))


def test_pvalues_and_bh_of_the_recorded_table_are_the_references():
    g = np.load(GOLDEN)
    tc = g["tab_cand"]
    assert not R.near_tie(g["ref_obs_loglk"][tc], g["umis"][tc], g["tab_n"], g["tab_loglk"])
    p = R.ambient_pvalues(g["umis"][tc], g["ref_obs_loglk"][tc], g["tab_n"], g["tab_loglk"])
    assert np.array_equal(p, g["tab_pvalues"]) and np.array_equal(R.adjust_pvalue_bh(p), g["tab_pvalues_adj"])
    step = np.diff(g["tab_n"])
    assert (step == 1).any() and ((step >= 2) & (step < 20)).any() and ((step >= 20) & (step < 1000)).any() and (step >= 1000).any()


@pytest.mark.parametrize("seed,s,n", [(0, 0, 1), (0, 0, 9), (7, 3, 1001), (2 ** 63 + 5, 499, 64), (2 ** 64 - 1, 2 ** 40, 5)])
def test_philox_equals_numpys(seed, s, n):
    ref = np.random.Philox(counter=np.array([0, s, 0, 0], np.uint64), key=np.array([seed, 0], np.uint64)).random_raw(n)
    assert np.array_equal(R.philox_words(seed, s, n), ref)


def test_simulated_loglk_is_the_multinomial_logpmf():
    """the per-draw form of the simulation equals the closed form on the counts, and the draws nest"""
    from scipy.special import gammaln

    p = np.array([0.5, 0.2, 0.2, 0.05, 0.05])
    n, tab = R.simulate_philox(p, np.array([3, 10, 11, 400]), 4, seed=9)
    assert list(n) == [3, 10, 11, 400] and tab.shape == (4, 4)
    cdf = np.cumsum(p) / np.cumsum(p)[-1]
    for s in range(4):
        u = (R.philox_words(9, s, 400) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
        feat = np.searchsorted(cdf, u, side="right")
        for i, N in enumerate(n):
            c = np.bincount(feat[:N], minlength=5)
            want = gammaln(N + 1) + np.sum(c * np.log(p) - gammaln(c + 1))
            assert abs(tab[i, s] - want) <= 1e-12 * abs(want)
