"""GPU tests of the JIBES tag caller (Context.jibes_tag_counts / jibes_fit / multigenome_jibes, engine.call_tags_jibes).

The expected values come from tests/jibes_numpy.py, the numpy restatement of lib/rust/jibes_o3/src/lib.rs, run on the fixtures of
tests/golden/jibes_reference.npz (tests/test_jibes_restatement.py says how they were recorded and pins the restatement itself); a
fixture's restatement is computed once per session and shared.  Equal: iterations, converged, z, k_let_limited, every assignment code
and, for the Multiplets, the most likely multiplet state, outside the barcodes the file lists as too close to a threshold or a tie (at
most 1 %; none in the recorded fixtures).  Within jibes_bound, read from the file and nowhere else (16 x the restatement's own movement
under permutations of the barcodes and +-1 ulp in exp and log): the model and LL relatively, the probabilities and the posterior
absolutely.  Bit for bit: run against run, CRGPU_JIBES_BATCH = 1 and 7 against the default, with and without the posterior output."""
import numpy as np
import pytest

import jibes_numpy as R
import multigenome_numpy as MG
from test_jibes_restatement import fixture_fit, golden

pytestmark = pytest.mark.gpu
EINVAL, ERANGE = -1, -6
_CTX = []


def ctx():
    import gpu_helpers as G

    if not _CTX:
        _CTX.append(G.fresh_ctx())
    return _CTX[0]


def _fit(c, name, run=0, **kw):
    g = golden()
    tol = g[name + "_tols"][run]
    args = dict(n_gems=int(g[name + "_n_gems"]), estimated_cells=float(g[name + "_estimated_cells"]), abs_tol=float(tol[0]), rel_tol=float(tol[1]),
                max_reps=int(g[name + "_max_reps"]), want_posterior=True)
    args.update(kw)
    return c.jibes_fit(g[name + "_Y"], g[name + "_bg0"], g[name + "_fg0"], g[name + "_sd0"], **args)


def _bits(fit):
    keys = ("bg", "fg", "sd", "LL", "iterations", "converged", "n_states", "k_let_limited", "probs", "assignment", "assignment_prob", "ml_state", "posterior")
    return {k: np.asarray(fit[k]).tobytes() for k in keys if k in fit}


def _against_restatement(name, got, ref, exclude_blanks):
    g = golden()
    bound = float(g["jibes_bound"])
    n, k = g[name + "_Y"].shape
    assert (got["iterations"], got["converged"], got["n_states"], got["k_let_limited"]) == (ref["iterations"], ref["converged"], len(ref["states"]), ref["limited"])
    assert np.array_equal(got["states"], ref["states"])
    worst = {}
    for key in ("bg", "fg", "sd"):
        worst[key] = float(np.max(np.abs(got[key] - ref[key]) / np.abs(ref[key])))
    worst["LL"] = abs(got["LL"] - ref["LL"]) / abs(ref["LL"])
    worst["posterior"] = float(np.max(np.abs(got["posterior"] - ref["posterior"])))
    tab = R.assignment_table(ref["posterior"], ref["states"], 0.9, exclude_blanks)
    worst["probs"] = float(np.max(np.abs(got["probs"] - tab["probs"])))
    worst["assignment_prob"] = float(np.max(np.abs(got["assignment_prob"] - tab["probability"])))
    print(name, "iterations", got["iterations"], "bound", bound, "largest differences", worst)
    assert not np.isnan(got["posterior"]).any() and not np.isnan(got["probs"]).any()
    ninf = np.isneginf(ref["prior"])
    assert np.array_equal(ninf, np.isneginf(got["prior"])) and np.all(got["posterior"][:, ninf] == 0.0)
    assert all(v <= bound for v in worst.values()), (worst, bound)
    keep = np.setdiff1d(np.arange(n), g[name + "_excluded"])
    assert np.array_equal(got["assignment"][keep], tab["assignment"][keep])
    mult = keep[tab["assignment"][keep] == k]
    assert np.array_equal(got["ml_state"][mult], tab["ml_state"][mult])
    return tab


@pytest.mark.parametrize("name,run", [("f65", 0), ("f400", 0), ("f400", 1), ("f1000", 0), ("f1000", 1), ("f130", 0), ("f1", 0)])
def test_fixture_equals_the_restatement(name, run):
    ref = fixture_fit(name, run)
    got = _fit(ctx(), name, run, exclude_blanks_from_posterior=(run == 1))
    _against_restatement(name, got, ref, run == 1)
    if name == "f400":
        assert got["fg"][2] == 0.01 and int(np.isneginf(got["prior"]).sum()) == 11      # the clamp, exactly; the -inf priors
    if name == "f130":
        assert got["n_states"] == 970
    if name == "f65":
        assert got["n_states"] == 6 and not got["k_let_limited"]


def test_no_barcodes():
    got = ctx().jibes_fit(np.zeros((0, 3)), [1.0, 1.0, 1.0], [0.5, 0.5, 0.5], [0.3, 0.3, 0.3], n_gems=2000, estimated_cells=0.0, want_posterior=True)
    ref = R.perform_em(np.zeros((0, 3)), R.generate_all_multiplets(3, 2), None, [1.0] * 3, [0.5] * 3, [0.3] * 3)
    assert got["LL"] == 0.0 == ref["LL"] and got["converged"] and got["iterations"] == 0 and list(got["fg"]) == [0.0] * 3 == list(ref["fg"])
    assert list(got["bg"]) == [1.0] * 3 and got["probs"].shape == (0, 5) and got["posterior"].shape[0] == 0


@pytest.mark.parametrize("name", ["f400", "f130"])
def test_bit_for_bit_between_runs_batches_and_outputs(name, monkeypatch):
    import gpu_helpers as G

    monkeypatch.delenv("CRGPU_JIBES_BATCH", raising=False)
    first = _fit(ctx(), name)
    again = _fit(ctx(), name)
    assert _bits(first) == _bits(again)
    lean = _fit(ctx(), name, want_posterior=False)
    assert "posterior" not in lean and _bits(lean) == {k: v for k, v in _bits(first).items() if k != "posterior"}
    for batch in ("1", "7"):      # read when the context is created
        monkeypatch.setenv("CRGPU_JIBES_BATCH", batch)
        c = G.fresh_ctx()
        assert _bits(_fit(c, name)) == _bits(first), batch
        c.close()


@pytest.mark.parametrize("name", ["f400", "f1000"])
def test_max_reps_below_convergence(name):
    g = golden()
    got = _fit(ctx(), name, max_reps=5)
    bound = float(g["jibes_bound"])
    assert not got["converged"] and got["iterations"] == int(g[name + "_reps5_iterations"]) == 6 and not bool(g[name + "_reps5_converged"])
    for key in ("bg", "fg", "sd"):
        assert np.all(np.abs(got[key] - g["%s_reps5_%s" % (name, key)]) <= bound * np.abs(g["%s_reps5_%s" % (name, key)])), key
    assert abs(got["LL"] - float(g[name + "_reps5_LL"])) <= bound * abs(float(g[name + "_reps5_LL"]))
    ref = fixture_fit(name, 0, max_reps=5)
    assert ref["iterations"] == 6 and np.max(np.abs(got["posterior"] - ref["posterior"])) <= bound


def _matrix(c, dense_by_column, n_features):
    """MatrixDev of V columns (the k-th whitelist entry each) from a dense V x n_features table"""
    V = len(dense_by_column)
    c.set_whitelist(0, np.arange(max(4096, V), dtype=np.uint32), length=16)
    seen = np.zeros(c.n_canon, np.uint32)
    seen[:V] = 1
    c.set_counts(0, 0, seen)
    cols, rows = np.nonzero(dense_by_column)
    m = c.assemble_matrix_dev(c.upload(cols.astype(np.uint32)), c.upload(rows.astype(np.uint32)), c.upload(dense_by_column[cols, rows].astype(np.uint32)),
                              len(cols))
    assert m.n_barcodes == V
    return m


def test_tag_table():
    import gpu_helpers as G
    from cellranger_amd import engine as E

    c = G.fresh_ctx()
    rng = np.random.RandomState(21)
    V, NF = 300, 23
    tag_rows = np.array([2, 5, 6, 11, 22], np.uint32)      # interleaved with gene rows
    dense = rng.poisson(0.5, (V, NF)) * rng.randint(1, 400, (V, NF))
    dense[7] = 0                                            # an empty column
    dense[8, tag_rows] = 0                                  # genes only
    dense[9, tag_rows] = [3, 0, 4, 5, 0]                    # exactly 12
    dense[10, tag_rows] = [3, 0, 4, 5, 1]                   # 13
    dense[11, tag_rows] = [0, 0, 0, 13, 0]                  # 13, all of it in the tag that is dropped afterwards
    valid = np.array([1, 1, 1, 0, 1], bool)
    m = _matrix(c, dense, NF)
    tab = c.jibes_tag_counts(m, tag_rows, NF)
    sums, nz, kept, logs = R.tag_table(dense[:, tag_rows], valid)
    assert np.array_equal(tab["counts"], dense[:, tag_rows]) and np.array_equal(tab["row_sums"], sums.astype(np.uint64))
    assert np.array_equal(tab["near_zero"], nz) and np.array_equal(tab["kept"], kept)
    assert {7, 8, 9} <= set(nz.tolist()) and {10, 11} <= set(kept.tolist())
    assert tab["log_counts"][kept][:, valid].tobytes() == logs.tobytes()
    for bad, code in ((tag_rows[::-1].copy(), EINVAL), (np.array([2, 5, 5], np.uint32), EINVAL), (np.array([2, NF], np.uint32), EINVAL)):
        with pytest.raises(E.CrgpuError) as ei:
            c.jibes_tag_counts(m, bad, NF)
        assert ei.value.code == code
    c.close()
    # one column per count 0 .. 70 000: the logarithm is numpy's, bit for bit
    c = G.fresh_ctx()
    sweep = np.arange(70001, dtype=np.int64)[:, None]
    ms = _matrix(c, sweep, 1)
    t = c.jibes_tag_counts(ms, np.array([0], np.uint32), 1)
    assert np.array_equal(t["counts"][:, 0], sweep[:, 0]) and t["log_counts"][:, 0].tobytes() == np.log10(sweep[:, 0] + 1.0).tobytes()
    assert np.array_equal(t["near_zero"], np.arange(13)) and len(t["kept"]) == 70001 - 13
    c.close()


def test_argument_checks():
    from cellranger_amd import engine as E

    c = ctx()
    y = np.ones((5, 17))
    for kw, yy, k, code in ((dict(), y, 17, ERANGE), (dict(max_k_lets=4), y[:, :3], 3, ERANGE)):
        with pytest.raises(E.CrgpuError) as ei:
            c.jibes_fit(yy, [1.0] * k, [0.5] * k, [0.3] * k, n_gems=2000, estimated_cells=5.0, **kw)
        assert ei.value.code == code
    with pytest.raises(E.CrgpuError) as ei:      # the Rust asserts it
        c.jibes_fit(y[:, :3], [1.0] * 3, [0.5, 0.009, 0.5], [0.3] * 3, n_gems=2000, estimated_cells=5.0)
    assert ei.value.code == EINVAL and "foreground" in str(ei.value)


def test_call_tags_jibes_end_to_end():
    """the k = 3 fixture as a filtered matrix: its tags on rows 1, 4 and 6 among gene rows, a fourth tag row that is not valid, and
    near-zero barcodes mixed in"""
    import gpu_helpers as G
    from cellranger_amd import engine as E

    g = golden()
    counts = g["f400_counts"]
    n = len(counts)
    rng = np.random.RandomState(31)
    V, NF = n + 9, 9
    pos = np.sort(rng.choice(V, n, replace=False))            # where the fixture's barcodes sit
    tag_rows = np.array([1, 4, 6, 7], np.uint32)
    dense = np.zeros((V, NF), np.int64)
    dense[:, [0, 2, 3, 5, 8]] = rng.poisson(3.0, (V, 5))
    dense[pos[:, None], tag_rows[None, :3]] = counts
    near = np.setdiff1d(np.arange(V), pos)
    dense[near[:4], 4] = [0, 5, 12, 1]                        # near zero: at most 12 over ALL tag rows
    dense[near[4:], 7] = [2, 12, 0, 7, 1]
    assert np.all(dense[pos][:, tag_rows].sum(axis=1) > 12)
    valid = [True, True, True, False]
    prelim = np.full(V, -1, np.int32)
    prelim[pos] = np.argmax(counts, axis=1)                   # a marginal caller's call, as good as any
    prelim[pos[::7]] = -1
    c = G.fresh_ctx()
    m = _matrix(c, dense, NF)
    est = float(g["f400_estimated_cells"])
    got = E.call_tags_jibes(c, m, tag_rows, valid, prelim, throughput="LT", n_gems=2000, n_features=NF, estimated_cells=est, tag_names=[b"CMO1", "CMO2", "CMO3", "CMO4"],
                            confidence=0.5)      # the synthetic well is noisy: at 0.9 nearly every barcode is Unassigned and none a Multiplet
    ref = R.call_tags(dense[:, tag_rows], valid, prelim, 2000, confidence=0.5, estimated_cells=est)
    assert np.array_equal(got["kept"], pos) and np.array_equal(got["near_zero"], near) and np.array_equal(ref["kept"], pos)
    assert got["fit"]["iterations"] == ref["fit"]["iterations"] and got["fit"]["converged"]
    assert sorted(got["snr"]) == ["snr_CMO1", "snr_CMO2", "snr_CMO3"] and list(got["barcodes_per_tag"]) == ["CMO1", "CMO2", "CMO3"]
    bound = float(g["jibes_bound"])
    for t, nm in enumerate(("CMO1", "CMO2", "CMO3")):
        assert got["barcodes_per_tag"][nm] == ref["per_tag"][t], nm
        assert abs(got["snr"]["snr_" + nm] - ref["snr"][t]) <= 2 * bound * abs(ref["snr"][t])      # a quotient of two bounded numbers
    assert got["non_singlets"] == ref["non_singlets"] and got["non_singlets"]["Blank"][-len(near):] == near.tolist()
    assert len(got["non_singlets"]["Multiplet"]) > 0 and sum(len(v) for v in got["barcodes_per_tag"].values()) > 0
    c.close()


def test_multigenome_jibes():
    """the k = 2 shape: the fixture's counts as the UMI totals over two genomes"""
    g = golden()
    c0, c1 = g["f65_counts"][:, 0].astype(np.int64), g["f65_counts"][:, 1].astype(np.int64)
    first = MG.classify(c0, c1)[0]
    assert len(set(first.tolist())) > 1
    y = np.stack((np.log10(c0 + 1.0), np.log10(c1 + 1.0)), axis=1)
    calls = np.where(first == MG.GENOME0, 0, np.where(first == MG.GENOME1, 1, -1))
    bg, fg, sd = R.initial_parameters(y, calls)
    states, limited, _, mmk, est = R.latent_state_setup(len(y), 2, 2000)
    ref = R.perform_em(y, states, R.log_prior(states, est, 2000, limited, mmk), bg, fg, sd)
    tab = R.assignment_table(ref["posterior"], states, apply_confidence=False)
    srt = np.sort(tab["probs"], axis=1)
    assert np.all(srt[:, -1] - srt[:, -2] >= 1e-9)      # no call of the restatement hangs on a tie
    m, inferred, call = ctx().multigenome_jibes(c0, c1, n_gems=2000)
    a = tab["assignment"]
    assert m == int((a == 2).sum()) and inferred == MG.infer(m, int((a == 0).sum()), int((a == 1).sum()))
    assert np.array_equal(call[a <= 2], np.array([MG.GENOME0, MG.GENOME1, MG.MULTIPLET])[a[a <= 2]]) and np.all(call[a == 3] == 255)
    one = ctx().multigenome_jibes(np.array([50, 60, 70]), np.array([0, 1, 2]), n_gems=2000)      # one class only: the early return
    assert one[0] == 0 and one[1] == 0.0 and len(set(one[2].tolist())) == 1


def test_close_shared_context():
    if _CTX:
        _CTX.pop().close()
