"""The numpy restatement of the JIBES tag caller (tests/jibes_numpy.py) against tests/golden/jibes_reference.npz.  No GPU.

How the golden file was recorded (once, by a throw-away script outside the repository, under numpy 2 / scipy 1.15 with np.NINF and
np.math shimmed back in; the file holds arrays only):
  states_*        cellranger.analysis.combinatorics.generate_all_multiplets_as_array, imported as it is;
  mcu_*, ec_*     get_multiplet_counts_unrounded and calculate_expected_total_cells of cellranger/feature/feature_assigner.py, copied
                  literally into the script (the module cannot be imported whole: it pulls in h5py through cellranger.matrix);
                  ec_solver_diff = the restatement's bisection minus scipy's BFGS stopping point;
  estep*          JibesEMPy._calculate_latent_state_weights / _calculate_posterior_by_state of cellranger/analysis/jibes_py.py, imported
                  with statsmodels and feature_assigner stubbed (the copies above stand in for the latter); cases 1 and 4 are limited
                  models with k <= 3 and carry the -inf priors, where the Python and the Rust agree;
  init*           cellranger.analysis.jibes.create_initial_parameters, imported with its heavy imports stubbed and a plain record for
                  JibesModelO3;
  f65 .. f1       seeded synthetic wells (counts, log10 table, initial model, the REFERENCE's estimated_cells) with the restatement's own
                  outputs: iterations, the LL trajectory, the model, the assignment tables, the head of the posterior; <fixture>_movement
                  = the largest relative change of model and LL and absolute change of the posterior over 8 seeded permutations of
                  the barcodes and 8 seeded runs in which every exp and log result of the E step is moved by -1, 0 or +1 ulp (the
                  iteration counts did not change in any of them); jibes_movement = the largest of these over the fixtures and their
                  tolerance pairs (1.27e-13, the 16-tag fixture), ONE number as the float bound is one number; jibes_bound = 16 x
                  jibes_movement = 2.03e-12, the factor the enrichment fit used.  The bound is read from the file only.  A bound per
                  fixture would not mean much for n = 1: a permutation of one barcode moves nothing, so that fixture's own figure
                  (7e-16) does not see the order of the sums at all, while its residual (c1 x + c0) - y cancels to about 0.005 of y.

Tolerances that are not equality.  The Poisson counts: exp(k ln mu - lgamma(k + 1) - mu) here against scipy's pmf; the exponent is at
most about 64 in magnitude and each of its three terms is rounded, so the results agree to 3 x 64 x 2^-53 plus the two libraries' exp
and lgamma errors: 1e-13 relative is asserted.  The E step against the Python: its sum over tags runs in another order than prior +
tag by tag; log densities of a few hundred in magnitude carry about 1e-13 of rounding, which the exponential turns into a relative
1e-13 of a posterior <= 1 and the log-sum into 1e-13 of LL: 1e-12 absolute on the posterior and the prior, 1e-12 relative on LL."""
import math
import os

import numpy as np
import pytest

import jibes_numpy as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "jibes_reference.npz")
FIXTURES = ["f65", "f400", "f1000", "f130", "f1"]
_G = {}
_FIT = {}


def golden():
    if not _G:
        _G.update(np.load(GOLDEN))
    return _G


def fixture_fit(name, run=0, max_reps=None):
    """the restatement on a fixture, computed once per (fixture, run) and shared (tests/test_gpu_jibes.py reads it too)"""
    key = (name, run, max_reps)
    if key not in _FIT:
        g = golden()
        Y, ng, est = g[name + "_Y"], int(g[name + "_n_gems"]), float(g[name + "_estimated_cells"])
        states, limited, _, mmk, _ = R.latent_state_setup(len(Y), Y.shape[1], ng, estimated_cells=est)
        prior = R.log_prior(states, est, ng, limited, mmk)
        tol = g[name + "_tols"][run]
        fit = R.perform_em(Y, states, prior, g[name + "_bg0"], g[name + "_fg0"], g[name + "_sd0"], abs_tol=tol[0], rel_tol=tol[1],
                           max_reps=int(g[name + "_max_reps"]) if max_reps is None else max_reps)
        fit.update(states=states, prior=prior, limited=limited)
        _FIT[key] = fit
    return _FIT[key]


@pytest.mark.parametrize("k", [1, 2, 3, 12, 16])
def test_latent_states_equal_the_reference(k):
    g = golden()
    for m, lim in ((3, 1), (3, 0), (2, 0)):
        a = R.generate_all_multiplets(k, m, bool(lim))
        assert a.dtype == np.int32 and np.array_equal(a, g["states_k%d_m%d_lim%d" % (k, m, lim)])
    assert len(R.generate_all_multiplets(16, 3, True)) == 970 and len(R.generate_all_multiplets(12, 3, True)) == 456


def test_poisson_counts_and_expected_cells():
    g = golden()
    for (x, ng), want in zip(g["mcu_cases"], g["mcu_expect"]):
        got = R.multiplet_counts_unrounded(x, int(ng))
        assert got.shape == (14,) and np.all(np.abs(got - want) <= 1e-13 * np.abs(want))
    for (n, ng), want, diff in zip(g["ec_cases"], g["ec_expect"], g["ec_solver_diff"]):
        got = R.expected_total_cells(int(n), int(ng))
        # the root against BFGS's stopping point: what the recording measured (at most 2.4e-6 cells), with room for another libm
        assert abs((got - want) - diff) <= 1e-9 * want and abs(got - want) <= 1e-5
        assert abs(float(np.sum(R.multiplet_counts_unrounded(got, int(ng)))) - n) <= 1e-9 * n      # it IS the root
    with pytest.raises(R.CellEstimateCantConverge):
        R.expected_total_cells(70000, 95000)      # the reference raises there too (recorded)


def test_e_step_equals_the_python_original():
    g = golden()
    seen_inf = 0
    for ci in range(int(g["estep_n_cases"])):
        p = "estep%d_" % ci
        Y, ng, est = g[p + "Y"], int(g[p + "n_gems"]), float(g[p + "estimated_cells"])
        states, limited, _, mmk, _ = R.latent_state_setup(len(Y), Y.shape[1], ng, estimated_cells=est)
        assert np.array_equal(states, g[p + "states"]) and limited == bool(g[p + "limited"]) and mmk == int(g[p + "max_modeled"])
        prior = R.log_prior(states, est, ng, limited, mmk)
        fin = np.isfinite(g[p + "prior"])
        assert np.array_equal(fin, np.isfinite(prior)) and np.all(np.isneginf(prior[~fin]))
        assert np.all(np.abs(prior[fin] - g[p + "prior"][fin]) <= 1e-12)
        seen_inf += int((~fin).sum())
        if Y.shape[1] <= 3 and limited:      # the quirk: the 3-lets index the overwritten, empty last entry
            assert np.array_equal(~fin, states.sum(axis=1) == mmk)
        P, LL = R.e_step(Y, states, prior, g[p + "bg"], g[p + "fg"], g[p + "sd"])
        assert not np.isnan(P).any() and np.all(P[:, ~fin] == 0.0)
        assert np.all(np.abs(P - g[p + "posterior"]) <= 1e-12) and abs(LL - float(g[p + "LL"])) <= 1e-12 * abs(float(g[p + "LL"]))
    assert seen_inf > 0


def test_m_step_is_the_weighted_least_squares_of_the_tiled_design():
    """JibesEMPy._maximize_parameters: WLS of the tiled data on [1, x_k] with the flattened posterior as weights.  On unclamped
    cases the closed form equals np.linalg.lstsq on the whitened design; lstsq (SVD) and the normal equations agree to about
    cond^2 eps, here below 1e-9."""
    rng = np.random.RandomState(3)
    for n, k, m in ((5, 2, 2), (7, 3, 2), (4, 2, 3)):
        states = R.generate_all_multiplets(k, m, False)
        z = len(states)
        truth = rng.randint(0, z, n)
        truth[:2] = [0, z - 1]      # some spread in every tag
        P = 0.3 * rng.dirichlet(np.ones(z), n)      # weights that lean on the state the data were drawn from: an unclamped slope
        P[np.arange(n), truth] += 0.7
        truth_b, truth_f = rng.uniform(0.5, 1.5, k), rng.uniform(0.5, 1.5, k)
        Y = truth_b + truth_f * states[truth] + rng.normal(0, 0.1, (n, k))
        bg, fg, sd = R.m_step(Y, states, P)
        W = np.sqrt(P.flatten())
        for t in range(k):
            X = np.stack((np.ones(n * z), np.tile(states[:, t].astype(float), n)), axis=1)
            yy = np.repeat(Y[:, t], z)
            coef = np.linalg.lstsq(X * W[:, None], yy * W, rcond=None)[0]
            assert coef[1] >= 0.01
            assert abs(coef[0] - bg[t]) <= 1e-9 and abs(coef[1] - fg[t]) <= 1e-9
            res = np.sum(P.flatten() * (X @ np.array([bg[t], fg[t]]) - yy) ** 2)
            assert abs(sd[t] - math.sqrt(res / P.sum())) <= 1e-12


def test_m_step_clamp_and_sd_floor_by_hand():
    # two states (blank, one tag), two barcodes, equal weights 1/2: x_bar = 1/2; y does not depend on x -> slope 0 -> clamped
    states = np.array([[0], [1]], np.int32)
    P = np.full((2, 2), 0.5)
    Y = np.array([[1.0], [3.0]])
    bg, fg, sd = R.m_step(Y, states, P)
    assert fg[0] == 0.01 and bg[0] == 2.0 - 0.01 * 0.5      # the intercept re-estimated: y_bar - 0.01 x_bar
    want = math.sqrt((0.5 * ((bg[0] - 1) ** 2 + (bg[0] + 0.01 - 1) ** 2 + (bg[0] - 3) ** 2 + (bg[0] + 0.01 - 3) ** 2)) / 2.0)
    assert abs(sd[0] - want) <= 1e-15
    # a perfect fit: barcode 0 is surely blank, barcode 1 surely the tag; y = 1 + 2 x exactly -> residual 0 -> the floor
    P = np.array([[1.0, 0.0], [0.0, 1.0]])
    bg, fg, sd = R.m_step(Y, states, P)
    assert (bg[0], fg[0], sd[0]) == (1.0, 2.0, 0.0001)


def test_em_loop_rules():
    states = R.generate_all_multiplets(2, 2, False)
    prior = R.log_prior(states, 30.0, 2000, False, 2)
    rng = np.random.RandomState(5)
    Y = rng.uniform(0.5, 3.0, (30, 2))
    args = (Y, states, prior, [1.0, 1.0], [1.0, 1.0], [0.5, 0.5])
    assert R.perform_em(*args, max_reps=0)["iterations"] == 1 and not R.perform_em(*args, max_reps=0)["converged"]
    r = R.perform_em(*args, max_reps=3, abs_tol=-1.0, rel_tol=-1.0)      # never converges: max_reps + 1 steps run
    assert r["iterations"] == 4 and not r["converged"] and len(r["lls"]) == 5
    r = R.perform_em(*args, abs_tol=1e9)      # the first comparison is at rep 2: never against the initial -inf
    assert r["iterations"] == 2 and r["converged"]
    e = R.perform_em(np.zeros((0, 2)), states, prior, [1.0, 1.0], [1.0, 1.0], [0.5, 0.5])
    assert e["LL"] == 0.0 and e["converged"] and e["iterations"] == 0 and list(e["fg"]) == [0.0, 0.0]
    # strict: a change EQUAL to abs_tol does not stop (the Python original's <= would)
    lls = R.perform_em(*args, abs_tol=-1.0, rel_tol=-1.0, max_reps=6)["lls"]
    d = lls[2] - lls[1]
    assert R.perform_em(*args, abs_tol=d, rel_tol=-1.0, max_reps=6)["iterations"] > 2
    assert R.perform_em(*args, abs_tol=np.nextafter(d, np.inf), rel_tol=-1.0, max_reps=6)["iterations"] == 2


def test_initial_parameters_equal_the_reference():
    g = golden()
    assert int(g["init_n_cases"]) == 5
    for ci in range(5):
        p = "init%d_" % ci
        bg, fg, sd = R.initial_parameters(g[p + "Y"], g[p + "calls"])
        for got, key in ((bg, "bg"), (fg, "fg"), (sd, "sd")):
            assert got.tobytes() == g[p + key].tobytes(), (ci, key)
    assert list(g["init2_fg"]) == [1.0] * 3 and list(g["init2_bg"]) == [0.5] * 3 and list(g["init2_sd"]) == [0.3] * 3
    assert g["init3_sd"][2] == 0.2 and np.all(g["init0_fg"] >= 0.6 - 1e-15)


def test_assignment_semantics_by_hand():
    states = R.generate_all_multiplets(2, 2, False)      # blank, 01, 10, 02, 11, 20
    assert R.state_classes(states).tolist() == [3, 1, 0, 1, 2, 0]
    post = np.array([[0.0, 0.25, 0.25, 0.0, 0.5, 0.0],      # tag0 0.25, tag1 0.25, Multiplet 0.5
                     [0.0, 0.2, 0.5, 0.1, 0.0, 0.2],        # tag0 0.7 (1-let + 2-let of the same tag), tag1 0.3
                     [0.5, 0.0, 0.5, 0.0, 0.0, 0.0],        # a tie of tag0 and Blank: the first in the order tags, Multiplet, Blank
                     [0.08, 0.0, 0.85, 0.0, 0.07, 0.0],     # 0.85 < 0.9 but 0.85 / 0.92 > 0.9
                     [0.95, 0.05, 0.0, 0.0, 0.0, 0.0]])     # Blank is never divided
    t = R.assignment_table(post, states, 0.9, False)
    assert t["candidate"].tolist() == [2, 0, 0, 0, 3] and t["assignment"].tolist() == [4, 4, 4, 4, 3]
    assert np.allclose(t["probs"][1], [0.7, 0.3, 0.0, 0.0]) and t["probability"].tolist() == [0.5, 0.7, 0.5, 0.85, 0.95]
    tx = R.assignment_table(post, states, 0.9, True)
    assert tx["assignment"].tolist() == [4, 4, 0, 0, 3]      # 0.5 / (1 - 0.5) = 1.0; 0.85 / 0.92 = 0.92...
    assert R.assignment_table(post, states, apply_confidence=False)["assignment"].tolist() == [2, 0, 0, 0, 3]
    assert t["ml_state"].tolist() == [4, 4, 4, 4, 4]
    three = R.generate_all_multiplets(3, 2, False)
    mcols = np.nonzero(R.state_classes(three) == 3)[0]
    p3 = np.zeros((1, len(three)))
    p3[0, mcols[1]] = p3[0, mcols[2]] = 0.5      # a tie of two multiplet states: the first
    t3 = R.assignment_table(p3, three, 0.9, False)
    assert t3["ml_state"][0] == mcols[1] and t3["assignment"][0] == 3
    per_tag, non = R.tag_assignments(t3, three, kept=[7], near_zero=[2, 9])
    assert non == {"Blank": [2, 9], "Unassigned": [], "Multiplet": [7]}
    assert [per_tag[i] for i in range(3)] == [[7] if three[mcols[1], i] > 0 else [] for i in range(3)]
    # the near-zero rule looks at ALL tags, before the invalid ones are dropped; 12 is near zero, 13 is not
    dense = np.array([[6, 6, 0], [6, 7, 0], [0, 0, 13], [1, 0, 11]])
    sums, nz, kept, logs = R.tag_table(dense, [True, True, False])
    assert sums.tolist() == [12, 13, 13, 12] and nz.tolist() == [0, 3] and kept.tolist() == [1, 2] and logs.shape == (2, 2)
    assert logs.tobytes() == np.log10(np.array([[7.0, 8.0], [1.0, 1.0]])).tobytes()


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_conditions_and_restatement(name):
    """the conditions a fixture was chosen for, from the file alone, and the restatement of today against the recorded one"""
    g = golden()
    n, k = g[name + "_Y"].shape
    bound = float(g["jibes_bound"])
    assert bound == R.BOUND_FACTOR * float(g["jibes_movement"]) and 0.0 < bound < 1e-11
    assert float(g["jibes_movement"]) == max(float(g[f + "_movement"]) for f in FIXTURES)
    assert np.array_equal(g[name + "_Y"], np.log10(g[name + "_counts"] + 1.0))
    ex = g[name + "_excluded"]
    assert len(ex) <= n // 100
    for ti, tol in enumerate(g[name + "_tols"]):
        q = "%s_run%d_" % (name, ti)
        lls = g[q + "lls"]
        assert len(lls) == int(g[q + "iterations"]) + 1 and bool(g[q + "converged"])
        for t in (len(lls) - 1, len(lls) - 2):      # the stopping change and the one before it, against both thresholds
            if t < 2:
                continue
            d, r = lls[t] - lls[t - 1], 1.0 - lls[t] / lls[t - 1]
            assert abs(d - tol[0]) >= float(g["stop_margin"]) * tol[0] and abs(r - tol[1]) >= float(g["stop_margin"]) * tol[1]
            assert ((d < tol[0]) or (r < tol[1])) == (t == len(lls) - 1)
        fit = fixture_fit(name, ti)
        assert fit["iterations"] == int(g[q + "iterations"]) and fit["converged"]
        for key in ("bg", "fg", "sd"):
            assert np.all(np.abs(fit[key] - g[q + key]) <= bound * np.abs(g[q + key])), key
        assert abs(fit["LL"] - lls[-1]) <= bound * abs(lls[-1])
        assert np.all(np.abs(fit["posterior"][:16] - g[q + "posterior_head"]) <= bound)
    fit = fixture_fit(name, 0)
    assert len(fit["states"]) == int(g[name + "_z"]) and fit["limited"] == bool(g[name + "_limited"])
    keep = np.setdiff1d(np.arange(n), ex)
    for nm, xb in (("tab", False), ("tabx", True)):
        t = R.assignment_table(fit["posterior"], fit["states"], 0.9, xb)
        p = t["probability"].copy()
        if xb:
            nb = t["candidate"] != k + 1
            p[nb] = p[nb] / (1.0 - t["probs"][nb, k + 1])
        srt = np.sort(g["%s_%s_probs" % (name, nm)], axis=1)
        assert np.all(np.abs(p[keep] - 0.9) >= float(g["conf_margin"])) and np.all((srt[:, -1] - srt[:, -2])[keep] >= float(g["max_margin"]))
        assert np.array_equal(t["assignment"][keep], g["%s_%s_assignment" % (name, nm)][keep])
        mult = keep[t["assignment"][keep] == k]
        assert np.array_equal(t["ml_state"][mult], g["%s_%s_ml_state" % (name, nm)][mult])
        assert np.all(np.abs(t["probs"] - g["%s_%s_probs" % (name, nm)]) <= bound)
    if name == "f400":
        assert fit["fg"][2] == 0.01 and int(np.isneginf(fit["prior"]).sum()) == 11
        assert np.all(fit["posterior"][:, np.isneginf(fit["prior"])] == 0.0) and not np.isnan(fit["posterior"]).any()
        assert 20 <= fit["iterations"] <= 25 and 38 <= fixture_fit(name, 1)["iterations"] <= 45
    if name == "f1000":
        assert len(fit["states"]) == 456 and 25 <= fit["iterations"] <= 35 and 50 <= fixture_fit(name, 1)["iterations"] <= 65
    if name == "f130":
        assert len(fit["states"]) == 970
    if name == "f65":
        assert len(fit["states"]) == 6 and not fit["limited"]
