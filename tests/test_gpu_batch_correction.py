"""GPU tests of CORRECT_CHEMISTRY_BATCH on the device (Context.knn_cross, engine.mnn_pairs, Context.batch_correct,
engine.batch_effect_score, engine.correct_chemistry_batch; csrc/knn.hip, csrc/batch_correction.hip).

Equal with NO tolerance to the reference as recorded in tests/golden/batch_correction_reference.npz and to the restatement
(tests/batch_correction_numpy.py), which the CPU tests pin to the reference: knn_cross's indices and distances on every fixture, the
mutual pairs, overlaps, align_orders and steps of engine.correct_chemistry_batch, the score before the correction, the NaN pattern, the
matrix of a schedule without steps.  knn_cross over the whole matrix with k + 1, minus its first column, is Context.knn.

Within a bound: the corr of every step and the aligned matrix against the exact (np.longdouble) answer.  The bound is 16 times the
deviation the f64 restatement itself shows from exact on that fixture (the largest over three pair orders, floored at one f64 rounding;
stored in the golden file): the project's rule for sseq and k-means.  The device differs from the restatement in its exp alone, which
is good to an ulp as numpy's is.  Measured on an MI355X, relative to the largest entry: corr of the stage fixtures at most 6.8e-15
(bounds 8.1e-14 to 1.7e-13), the aligned matrix at most 4.1e-15 (bounds 5.2e-15 to 9.5e-14 on the fixtures that move), the correction
fixtures at most 5.6e-15 (bounds 1.8e-15 to 8.9e-14; one_row_one_pair, where (w b) / w gives b back, 4.4e-20).

The score after the correction equals the restatement's score of the device's own aligned matrix, and the reference's recorded value
(every stored fixture passed the gap check of the golden script).

Bit for bit: run against run, every seam at its smallest and largest legal value, a sub-list of cur_rows against the same rows of the
whole, a schedule in one call against the same steps as single-step calls chained through the host.  Context.knn on an old fixture is
unchanged against tests/golden/knn_reference.npz.  The refusals with a live context, after which the context still works."""
import numpy as np
import pytest

import batch_correction_numpy as R
from test_batch_correction_restatement import GOLDEN, exact

pytestmark = pytest.mark.gpu
EINVAL = -1
_CTX = []


def ctx():
    import gpu_helpers as G

    if not _CTX:
        _CTX.append(G.fresh_ctx())
    return _CTX[0]


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def pair_tile_max(d, row_tile):
    """the largest legal pair_tile (include/crgpu.h): a multiple of 8 up to 64 that fits 72 KiB of LDS beside the rows; 0 = none"""
    have = 73728 // 8
    return 0 if row_tile * d >= have else min(64, (have - row_tile * d) // (d + row_tile) // 8 * 8)


_stage = {}


def staged(name):
    """engine.correct_chemistry_batch of a fixture, run once and shared"""
    from cellranger_amd import engine as E

    if name not in _stage:
        f = R.FIXTURES[name]
        _stage[name] = E.correct_chemistry_batch(ctx(), f["x"], f["batch_ids"], knn=f["knn"], alpha=f["alpha"], sigma=f["sigma"],
                                                 realign_panorama=f["realign_panorama"], n_batch_ids=f["n_batch_ids"])
    return _stage[name]


def in_batch_order(name, aligned):
    e = R.expected(name)
    return aligned[e["order"]] if e["need_reorder"] else aligned


@pytest.mark.parametrize("name", list(R.FIXTURES))
def test_knn_cross_equals_find_knn(golden, name):
    f, e = R.FIXTURES[name], R.expected(name)
    k = f["knn"]
    for (i, j), want in e["nn"].items():
        (lo_i, hi_i), (lo_j, hi_j) = e["ranges"][i], e["ranges"][j]
        r = ctx().knn_cross(e["x"], k, lo_i, hi_i - lo_i, lo_j, hi_j - lo_j)
        _, dist, _ = R.knn_cross(e["x"], k, lo_i, hi_i - lo_i, lo_j, hi_j - lo_j)
        assert r["indices"].dtype == np.int32 and np.array_equal(r["indices"], want), (i, j)
        assert np.array_equal(r["distances"], dist), (i, j)                                    # every bit, the root included
        assert np.array_equal(r["sorted_indices"], np.sort(want, axis=1))
        assert r["pairs_evaluated"] == (hi_i - lo_i) * (hi_j - lo_j)
        rows = golden["%s_nn_%d_%d_rows" % (name, i, j)]
        assert np.array_equal(r["indices"][rows], golden["%s_nn_%d_%d" % (name, i, j)]), (i, j)


def test_knn_cross_over_all_rows_is_knn_and_the_seams_move_no_bit():
    f, e = R.FIXTURES["two_d10"], R.expected("two_d10")
    x, n, k = e["x"], len(e["x"]), f["knn"]
    whole = ctx().knn_cross(x, k + 1, 0, n, 0, n)
    old = ctx().knn(x, k)
    assert np.array_equal(whole["indices"][:, 1:], old["indices"]) and np.array_equal(whole["distances"][:, 1:], old["distances"])
    assert np.array_equal(whole["indices"][:, 0], np.arange(n)) and not whole["distances"][:, 0].any()
    first = ctx().knn_cross(x, k, 0, 300, 300, 200)
    keys = ("indices", "distances", "sorted_indices")
    for kw in (dict(), dict(capacity=k + 4), dict(capacity=4096), dict(force_device=True), dict(cand_tile=4), dict(cand_tile=256)):
        got = ctx().knn_cross(x, k, 0, 300, 300, 200, **kw)
        assert all(got[key].tobytes() == first[key].tobytes() for key in keys), kw
    part = ctx().knn_cross(x, k, 100, 130, 300, 200)                   # a query range against the same rows of the whole
    assert all(part[key].tobytes() == np.ascontiguousarray(first[key][100:230]).tobytes() for key in keys)
    least = ctx().knn_cross(x, 200, 0, 3, 300, 200)                    # k = n_cands: every candidate, in order
    assert np.array_equal(least["sorted_indices"], np.tile(np.arange(300, 500), (3, 1)))


def test_knn_is_unchanged_on_an_old_fixture():
    import knn_numpy as K
    from test_knn_restatement import GOLDEN as KNN_GOLDEN

    g = np.load(KNN_GOLDEN)
    f = K.FIXTURES["n257"]
    r = ctx().knn(f["x"], f["k"])
    rows = g["n257_rows"]
    assert np.array_equal(r["indices"][rows], g["n257_ind"]) and np.array_equal(r["distances"][rows], g["n257_dist"])


@pytest.mark.parametrize("name", list(R.FIXTURES))
def test_stage_equals_the_reference(golden, name):
    from cellranger_amd import engine as E

    f, e, got = R.FIXTURES[name], R.expected(name), staged(name)
    assert list(got["mutual_nn"]) == list(e["mutual_nn"]) and got["ranges"] == e["ranges"] and got["need_reorder"] == e["need_reorder"]
    for key, pairs in e["mutual_nn"].items():
        assert got["mutual_nn"][key].dtype == np.int32 and np.array_equal(got["mutual_nn"][key], pairs), key
        assert np.array_equal(got["mutual_nn"][key], golden["%s_mnn_%d_%d" % (name, key[0], key[1])]), key
    assert list(got["overlap"].items()) == list(e["overlap"].items())
    assert np.array_equal(np.array(list(got["overlap"].values())), golden[name + "_overlap"])
    assert got["align_orders"] == e["align_orders"]
    assert np.array_equal(np.array(got["align_orders"], dtype=np.int32).reshape(-1, 2), golden[name + "_orders"])
    want_steps = [dict(ref_batches=s["ref_batches"], cur_batches=s["cur_batches"], n_cur=len(s["cur_rows"]), n_mnn=len(s["mnn_cur"])) for s in e["steps"]]
    assert got["steps"] == want_steps
    assert [(s["n_cur"], s["n_mnn"]) for s in got["steps"]] == [tuple(r) for r in golden[name + "_steps"].tolist()]
    aligned = in_batch_order(name, got["aligned"])
    if not e["steps"]:
        assert got["aligned"].tobytes() == f["x"].tobytes()                                   # nothing moves: bit for bit
    rows = golden[name + "_final_rows"]
    dev = R.rel_dev(aligned[rows], exact(golden, name + "_final"), float(golden[name + "_final_scale"]))
    bound = 16 * float(golden[name + "_dev_final"])
    print("%s: aligned %.3g from exact, bound %.3g" % (name, dev, bound))
    assert dev <= bound
    assert R.rel_dev(aligned, e["final"]) <= 2 * bound                                         # every row, against the restatement
    # the scores: before, with no tolerance; after, the restatement's score of the device's own matrix and the reference's value
    before = E.batch_effect_score(ctx(), e["x"], e["ids"], max_num_bcs=f["max_num_bcs"])
    after = E.batch_effect_score(ctx(), aligned, e["ids"], max_num_bcs=f["max_num_bcs"])
    assert before == e["score_before"] == float(golden[name + "_score_before"])
    assert after == R.batch_effect_score(aligned, e["ids"], max_num_bcs=f["max_num_bcs"]) == float(golden[name + "_score_after"])
    if f["max_num_bcs"] >= len(f["x"]):
        assert got["batch_score_before"] == before and got["batch_score_after"] == after


@pytest.mark.parametrize("name", [n for n in R.FIXTURES if R.expected(n)["steps"]])
def test_corr_of_every_step_against_exact(golden, name):
    f, e = R.FIXTURES[name], R.expected(name)
    r = ctx().batch_correct(e["x"], e["steps"], f["sigma"], want_corr=True)
    assert r["aligned"].tobytes() == np.ascontiguousarray(in_batch_order(name, staged(name)["aligned"])).tobytes()
    assert r["pairs_evaluated"] == sum(len(s["cur_rows"]) * len(s["mnn_cur"]) for s in e["steps"]) and r["zero_den_rows"] == 0
    assert r["chunks"] == sum(-(-len(s["mnn_cur"]) // R.PAIR_CHUNK) for s in e["steps"]) and r["step_ms"].shape == (len(e["steps"]), 4)
    bound = 16 * float(golden[name + "_dev_corr"])
    for s, corr in enumerate(r["corr"]):
        rows = golden["%s_corr%d_rows" % (name, s)]
        dev = R.rel_dev(corr[rows], exact(golden, "%s_corr%d" % (name, s)), float(golden["%s_corr%d_scale" % (name, s)]))
        print("%s step %d: corr %.3g from exact, bound %.3g" % (name, s, dev, bound))
        assert dev <= bound
        assert R.rel_dev(corr, e["corr"][s]) <= 2 * bound                                       # every row, against the restatement


def _correct(name, rows=None, **kw):
    f = R.CORRECTIONS[name]
    cur = f["cur_rows"] if rows is None else f["cur_rows"][rows]
    return ctx().batch_correct(f["x"], [(cur, f["mnn_cur"], f["mnn_ref"])], f["sigma"], want_corr=True, **kw)


_corrected = {}


def corrected(name):
    if name not in _corrected:
        _corrected[name] = _correct(name)
    return _corrected[name]


@pytest.mark.parametrize("name", list(R.CORRECTIONS))
def test_correction_fixture_against_exact(golden, name):
    f, r = R.CORRECTIONS[name], corrected(name)
    corr, want = r["corr"][0], R.expected_correction(name)
    assert np.array_equal(np.isnan(corr), np.isnan(want)) and np.array_equal(np.isnan(corr), np.isnan(golden[name + "_ref"]))
    dev, bound = R.rel_dev(corr, exact(golden, name)), 16 * float(golden[name + "_dev"])
    print("%s: corr %.3g from exact, bound %.3g" % (name, dev, bound))
    assert dev <= bound
    assert r["zero_den_rows"] == int(np.isnan(want).all(axis=1).sum()) == (1 if name == "nan_row" else 0)
    moved = f["x"].copy()
    moved[f["cur_rows"]] += corr
    assert r["aligned"].tobytes() == moved.tobytes()
    assert r["chunks"] == -(-len(f["mnn_cur"]) // R.PAIR_CHUNK) and r["pairs_evaluated"] == len(f["cur_rows"]) * len(f["mnn_cur"])
    if name == "nan_row":
        assert np.isnan(corr[33]).all() and np.isnan(r["aligned"][33]).all() and np.isfinite(np.delete(r["aligned"], 33, axis=0)).all()


@pytest.mark.parametrize("name", list(R.CORRECTIONS))
def test_bit_for_bit_between_runs_seams_and_sub_lists(name):
    f = R.CORRECTIONS[name]
    d, n_cur = f["x"].shape[1], len(f["cur_rows"])
    first = corrected(name)
    bits = (first["corr"][0].tobytes(), first["aligned"].tobytes())
    assert first["row_tile"] == 32 and first["pair_tile"] == pair_tile_max(d, 32)
    again = _correct(name)
    assert (again["corr"][0].tobytes(), again["aligned"].tobytes()) == bits
    for row_tile in (16, 32, 64):
        top = pair_tile_max(d, row_tile)
        if top < 8:
            continue
        for kw in (dict(pair_tile=8), dict(pair_tile=top), dict(pair_tile=8, slab_rows=row_tile), dict(pair_tile=top, slab_rows=2 * row_tile)):
            got = _correct(name, row_tile=row_tile, **kw)
            assert (got["corr"][0].tobytes(), got["aligned"].tobytes()) == bits, (row_tile, kw)
            assert got["row_tile"] == row_tile and got["pair_tile"] == kw["pair_tile"]
    if n_cur > 1:
        rows = np.arange(n_cur)[n_cur // 3:n_cur // 3 + max(1, n_cur // 2)][::-1]            # a sub-list, backwards
        part = _correct(name, rows=rows)
        assert part["corr"][0].tobytes() == np.ascontiguousarray(first["corr"][0][rows]).tobytes()


@pytest.mark.parametrize("name", ["three_d100", "four_panorama", "realign"])
def test_one_call_equals_the_steps_chained_through_the_host(name):
    f, e = R.FIXTURES[name], R.expected(name)
    whole = ctx().batch_correct(e["x"], e["steps"], f["sigma"], want_corr=True)
    x = e["x"]
    for s, st in enumerate(e["steps"]):
        one = ctx().batch_correct(x, [st], f["sigma"], want_corr=True, row_tile=16 if s % 2 else 64 if pair_tile_max(x.shape[1], 64) >= 8 else 32)
        assert one["corr"][0].tobytes() == whole["corr"][s].tobytes(), s
        x = one["aligned"]
    assert x.tobytes() == whole["aligned"].tobytes()


def test_num_pcs_is_a_view_and_no_step_returns_the_matrix():
    f = R.CORRECTIONS["three_chunks"]
    wide = np.ascontiguousarray(np.concatenate([f["x"], np.full((len(f["x"]), 3), np.inf)], axis=1))
    r = ctx().batch_correct(wide, [(f["cur_rows"], f["mnn_cur"], f["mnn_ref"])], f["sigma"], num_pcs=10, want_corr=True)
    assert r["corr"][0].tobytes() == corrected("three_chunks")["corr"][0].tobytes()
    none = ctx().batch_correct(wide, [], f["sigma"], num_pcs=10)
    assert none["aligned"].tobytes() == f["x"].tobytes() and none["pairs_evaluated"] == 0 and none["step_ms"].shape == (0, 4)


def test_score_refusals():
    from cellranger_amd import engine as E

    f = R.FIXTURES["two_d10"]
    assert np.isnan(E.batch_effect_score(ctx(), np.zeros((5, 2)), np.array([0, 0, 0, 0, 1])))
    with pytest.raises(ValueError):
        E.batch_effect_score(ctx(), f["x"], f["batch_ids"], knn_neighbors=1025)
    with pytest.raises(ValueError):
        E.batch_effect_score(ctx(), f["x"][:8], f["batch_ids"][[0, 1, 2, 3, 300, 301, 302, 303]], knn_neighbors=8)
    with pytest.raises(ValueError):
        E.correct_chemistry_batch(ctx(), f["x"], np.where(np.arange(500) < 495, 0, 1))        # a batch of 5 rows, knn = 10


def test_refusals_with_a_live_context():
    from cellranger_amd import _lib

    c = ctx()
    f = R.CORRECTIONS["three_chunks"]
    x, cur, mc, mr = f["x"], f["cur_rows"], f["mnn_cur"], f["mnn_ref"]
    for bad in (np.nan, np.inf, -np.inf):
        y = x.copy()
        y[169, 9] = bad
        with pytest.raises(_lib.CrgpuError) as e:
            c.batch_correct(y, [(cur, mc, mr)])
        assert e.value.code == EINVAL and "not finite" in str(e.value)
        with pytest.raises(_lib.CrgpuError) as e:
            c.knn_cross(y, 5, 0, 90, 90, 80)
        assert e.value.code == EINVAL and "not finite" in str(e.value)
    y = x.copy()
    y[5, 0] = np.nan                                                   # outside both ranges: not looked at
    assert np.array_equal(c.knn_cross(y, 5, 10, 80, 90, 80)["indices"], c.knn_cross(x, 5, 10, 80, 90, 80)["indices"])
    twice, outside = cur.copy(), mc.copy()
    twice[7], outside[4000] = twice[6], 170
    wide = np.zeros((10, 129))
    d128 = R.CORRECTIONS["d128"]
    for args, kw in ((([(twice, mc, mr)],), {}), (([(cur, outside, mr)],), {}), (([(cur, mc, -mr)],), {}), (([(cur, mc, mr)],), dict(sigma=-1.0)),
                     (([(cur, mc, mr)],), dict(sigma=np.inf)), (([(cur, mc[:0], mr[:0])],), {}), (([(cur[:0], mc, mr)],), {}),
                     (([(cur, mc, mr), (cur[:0], mc, mr)],), {}), (([(cur, mc, mr)],), dict(pair_tile=4)), (([(cur, mc, mr)],), dict(pair_tile=20)),
                     (([(cur, mc, mr)],), dict(pair_tile=72)), (([(cur, mc, mr)],), dict(row_tile=48)), (([(cur, mc, mr)],), dict(slab_rows=48)),
                     (([(cur, mc, mr)],), dict(num_pcs=0)), (([(cur, mc, mr[:-1])],), {})):
        with pytest.raises((_lib.CrgpuError, ValueError)) as e:
            c.batch_correct(x, *args, **kw)
        assert not isinstance(e.value, _lib.CrgpuError) or e.value.code == EINVAL, kw
    with pytest.raises(_lib.CrgpuError) as e:
        c.batch_correct(wide, [(np.arange(3), np.arange(3), np.arange(3))])
    assert e.value.code == EINVAL
    with pytest.raises(_lib.CrgpuError) as e:                          # 64 rows of 128 dimensions leave no room for a pair tile
        c.batch_correct(d128["x"], [(d128["cur_rows"], d128["mnn_cur"], d128["mnn_ref"])], row_tile=64)
    assert e.value.code == EINVAL
    for args, kw in (((x, 81, 0, 90, 90, 80), {}), ((x, 0, 0, 90, 90, 80), {}), ((x, 5, 0, 90, 90, 81), {}), ((x, 5, 100, 71, 0, 90), {}),
                     ((x, 5, 0, 0, 90, 80), {}), ((x, 5, 0, 90, 90, 0), {}), ((x, 5, 0, 90, 90, 80), dict(capacity=8)), ((x, 5, 0, 90, 90, 80), dict(cand_tile=6)),
                     ((x, 5, 0, 90, 90, 80), dict(num_pcs=11)), ((wide, 3, 0, 5, 5, 5), {})):
        with pytest.raises((_lib.CrgpuError, ValueError)) as e:
            c.knn_cross(*args, **kw)
        assert not isinstance(e.value, _lib.CrgpuError) or e.value.code == EINVAL, (args[1:], kw)
    assert _correct("three_chunks")["corr"][0].tobytes() == corrected("three_chunks")["corr"][0].tobytes()   # the context still works
