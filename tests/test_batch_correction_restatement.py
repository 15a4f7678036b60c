"""The numpy restatement of CORRECT_CHEMISTRY_BATCH (tests/batch_correction_numpy.py) against the reference's own outputs (no GPU).

tests/golden/batch_correction_reference.npz (scripts/make_batch_correction_golden.py) holds, per fixture, what the reference's find_knn,
correction_vector and batch_effect_score gave under scikit-learn 1.7.2 and what join()'s set arithmetic and panorama loop gave around
them, and the exact (np.longdouble) corrections as hi + lo.  Equal with NO tolerance: the neighbours, the mutual pairs, the overlaps,
align_orders, the steps and the score before the correction.  The corrections and the aligned matrix lie within the stored deviation
of exact (the restatement's own, the largest over three pair orders, floored at one f64 rounding) and within 1e-9 of the
reference's (scikit-learn expands the norm and lets BLAS order the sums; a wrong gamma, sign or swapped pair moves the answer by order
1).  The NaN rows agree."""
import os

import numpy as np
import pytest

import batch_correction_numpy as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "batch_correction_reference.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def exact(golden, key):
    return golden[key + "_hi"].astype(np.longdouble) + golden[key + "_lo"].astype(np.longdouble)


def test_longdouble_is_the_extended_format():
    assert np.finfo(np.longdouble).nmant == 63 and R.PAIR_CHUNK == 2048


@pytest.mark.parametrize("name", list(R.FIXTURES))
def test_stage_fixture_equals_the_reference(golden, name):
    f, e = R.FIXTURES[name], R.expected(name)
    nb = len(e["ranges"])
    for i in range(nb):
        for j in range(nb):
            if i != j:
                rows = golden["%s_nn_%d_%d_rows" % (name, i, j)]
                assert np.array_equal(e["nn"][(i, j)][rows], golden["%s_nn_%d_%d" % (name, i, j)]), (i, j)
    for (i, j), pairs in e["mutual_nn"].items():
        assert np.array_equal(pairs, golden["%s_mnn_%d_%d" % (name, i, j)]), (i, j)
    assert np.array_equal(np.array(list(e["overlap"].values())), golden[name + "_overlap"])
    assert np.array_equal(np.array(e["align_orders"], dtype=np.int32).reshape(-1, 2), golden[name + "_orders"])
    assert [(len(s["cur_rows"]), len(s["mnn_cur"])) for s in e["steps"]] == [tuple(r) for r in golden[name + "_steps"].tolist()]
    assert e["score_before"] == float(golden[name + "_score_before"])
    assert e["score_after"] == float(golden[name + "_score_after"])      # every stored fixture passed the gap check
    for s, corr in enumerate(e["corr"]):
        rows = golden["%s_corr%d_rows" % (name, s)]
        scale = float(golden["%s_corr%d_scale" % (name, s)])
        assert R.rel_dev(corr[rows], exact(golden, "%s_corr%d" % (name, s)), scale) <= float(golden[name + "_dev_corr"])
        assert R.rel_dev(corr[rows], golden["%s_corr%d_ref" % (name, s)], scale) <= 1e-9
    rows = golden[name + "_final_rows"]
    scale = float(golden[name + "_final_scale"])
    assert R.rel_dev(e["final"][rows], exact(golden, name + "_final"), scale) <= float(golden[name + "_dev_final"])
    assert R.rel_dev(e["final"][rows], golden[name + "_final_ref"], scale) <= 1e-9
    assert e["need_reorder"] == (name == "interleaved")
    if not e["steps"]:
        assert e["final"].tobytes() == f["x"].tobytes() and not e["align_orders"]


@pytest.mark.parametrize("name", list(R.CORRECTIONS))
def test_correction_fixture_equals_the_reference(golden, name):
    got = R.expected_correction(name)
    ref = golden[name + "_ref"]
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    assert R.rel_dev(got, exact(golden, name)) <= float(golden[name + "_dev"])
    assert R.rel_dev(got, ref) <= 1e-9
    assert np.isnan(got).any() == (name == "nan_row")


def test_the_fixtures_have_the_shapes_the_tests_need():
    e = R.expected("four_panorama")
    below = [k for k, v in e["overlap"].items() if v <= R.FIXTURES["four_panorama"]["alpha"]]
    assert below and all(k not in e["align_orders"] for k in below)
    two = [s for s in e["steps"] if len(s["cur_batches"]) == 2]
    assert two and (np.diff(two[0]["cur_rows"]) != 1).sum() == 1        # a two-batch panorama moves: two separate row ranges
    assert len(R.CORRECTIONS["three_chunks"]["mnn_cur"]) == 2 * R.PAIR_CHUNK + 609
    assert not R.expected("far_apart")["steps"]
    r = R.expected("realign")
    assert r["steps"][-1]["cur_batches"] == r["steps"][-1]["ref_batches"] == [0, 1, 2]
    f = R.FIXTURES["score_subsample"]
    xs, _, k = R.score_inputs(f["x"], f["batch_ids"], max_num_bcs=f["max_num_bcs"])
    assert len(xs) == 500 and k == 5 and len(np.unique(xs, axis=0)) < 500   # the subsample repeats rows
    assert np.isnan(R.batch_effect_score(np.zeros((5, 2)), np.array([0, 0, 0, 0, 1])))


def test_a_sub_list_of_cur_rows_gives_the_rows_of_the_whole():
    f = R.CORRECTIONS["three_chunks"]
    part = R.correction(f["x"], f["cur_rows"][10:30], f["mnn_cur"], f["mnn_ref"], f["sigma"])
    assert part.tobytes() == np.ascontiguousarray(R.expected_correction("three_chunks")[10:30]).tobytes()
