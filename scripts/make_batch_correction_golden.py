#!/usr/bin/env python
"""Record tests/golden/batch_correction_reference.npz: what the reference's own functions give on the fixtures of
tests/batch_correction_numpy.py, and the exact (np.longdouble) answers the device is measured against.

    python scripts/make_batch_correction_golden.py --reference DIR

DIR is a checkout of the reference; cellranger.analysis.batch_correction is imported from DIR/lib/python (scikit-learn 1.7.2, asserted).
The stage file imports martian and cannot be imported: join()'s loop is restated here around the reference's find_knn,
correction_vector and batch_effect_score, with Python sets as join() has them.

Per stage fixture <f> (a seeded sample of rows where an array would be large; never the fixture itself is cut):
  <f>_nn_<i>_<j>_rows, <f>_nn_<i>_<j>      find_knn of batch i in batch j (global indices) for sampled rows of batch i
  <f>_mnn_<i>_<j>, <f>_overlap, <f>_orders the mutual pairs (all, ascending), the overlaps in (i, j) order, align_orders
  <f>_steps                                per step n_cur, n_mnn
  <f>_corr<s>_rows, _ref, _hi, _lo, _scale correction_vector of step s on sampled cur rows: the reference's (from ITS chain's matrix),
                                           the exact one (from the longdouble chain) as hi + lo; max |corr| over ALL cur rows
  <f>_final_rows, _ref, _hi, _lo, _scale   the aligned matrix in batch order, likewise
  <f>_score_before, <f>_score_after        batch_effect_score of the reference on its own chain
  <f>_dev_corr, <f>_dev_final              the f64 restatement's deviation from exact, the largest over three pair orders (ascending,
                                           reversed, a seeded permutation), relative to max |corr| of the step / max |final|,
                                           and never below 2^-53: one rounding of the largest entry (where (w b) / w happens to
                                           give b back, the measured deviation says nothing about another exp's last bit)
Per correction fixture <c>: <c>_ref, <c>_hi, <c>_lo (all rows), <c>_dev.

A fixture is REJECTED when a cross query has two equal d2 among its first k + 1; when two overlaps, or an overlap and alpha, differ by
less than 1e-12 without being equal; when a row's den lies in (0, 1e-250); when on the original or the aligned matrix a score query's
d2 gap at the k boundary is below 1e-9 relative (copies of one row made by the subsample apart).  At most 1 in 8 may be rejected; the
count is printed and the seed of a rejected fixture is to be changed in tests/batch_correction_numpy.py.  scikit-learn's correction_vector
must lie within 1e-9 * max |corr| of the exact answer on every fixture: a condition (a wrong gamma, sign or swapped pair moves the answer
by order 1), not a tolerance."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import batch_correction_numpy as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "batch_correction_reference.npz")
SAMPLE_SEED = 20261020
NN_ROWS, CORR_ROWS, FINAL_ROWS = 16, 24, 32
LD = np.longdouble
ROUNDING = 2.0 ** -53   # no f64 result is expected nearer to exact than one rounding of its largest entry: the floor of a stored deviation


def sample(n, m, salt):
    if m >= n:
        return np.arange(n)
    rs = np.random.RandomState(SAMPLE_SEED + salt)
    return np.sort(np.concatenate([[0, n - 1], rs.choice(np.arange(1, n - 1), m - 2, replace=False)]))


def hi_lo(v):
    hi = np.asarray(v, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        lo = np.asarray(np.asarray(v, dtype=LD) - hi.astype(LD), dtype=np.float64)
    return hi, np.where(np.isfinite(hi), lo, 0.0)


def score_gap(x, ids, max_num_bcs):
    """the smallest relative d2 gap at the k boundary of batch_effect_score's query; a boundary between two copies of one row does not
    count (they share a batch id)"""
    got = R.score_inputs(x, ids, max_num_bcs=max_num_bcs)
    if got is None:
        return np.inf
    xs, _, k = got
    _, d2, first = R.knn_self(xs, k)
    a, b = d2[:, k], d2[:, k + 1]
    copies = (xs[first[:, k]] == xs[first[:, k + 1]]).all(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        gap = np.where(copies, np.inf, (b - a) / b)
    return float(gap.min())


def near(a, b):
    return a != b and abs(a - b) < 1e-12


def stage_fixture(name, f, ref, out):
    """-> the reason of a rejection, or None"""
    k, alpha, sigma = f["knn"], f["alpha"], f["sigma"]
    e = R.expected(name)
    x, ranges, ids = e["x"], e["ranges"], e["ids"]
    nb = len(ranges)
    # find_knn and the tie check
    nn_pairs = {}
    for i in range(nb):
        for j in range(nb):
            if i == j:
                continue
            (lo_i, hi_i), (lo_j, hi_j) = ranges[i], ranges[j]
            got = ref.find_knn(x[lo_i:hi_i], x[lo_j:hi_j], k).reshape(-1, k) + lo_j
            d2 = R.knn_cross(x, k, lo_i, hi_i - lo_i, lo_j, hi_j - lo_j)[2]
            if (np.diff(d2, axis=1) == 0).any():
                return "a cross query of (%d, %d) has equal d2 among its first k + 1" % (i, j)
            assert np.array_equal(got, e["nn"][(i, j)]), "%s: find_knn(%d, %d) differs from the restatement" % (name, i, j)
            rows = sample(hi_i - lo_i, NN_ROWS, 100 * i + j)
            out["%s_nn_%d_%d_rows" % (name, i, j)] = rows.astype(np.int32)
            out["%s_nn_%d_%d" % (name, i, j)] = got[rows].astype(np.int32)
            left = np.repeat(np.arange(lo_i, hi_i), k)
            nn_pairs[(i, j)] = set(zip(left.tolist(), got.ravel().tolist()))
    # join(): mutual_nn, overlap_percentage, align_orders
    mutual_nn, overlap = {}, {}
    for i in range(nb):
        for j in range(i + 1, nb):
            mutual_nn[(i, j)] = nn_pairs[(i, j)] & {(y, x_) for x_, y in nn_pairs[(j, i)]}
            overlap[(i, j)] = max(float(len({a for a, _ in mutual_nn[(i, j)]})) / (ranges[i][1] - ranges[i][0]),
                                  float(len({b for _, b in mutual_nn[(i, j)]})) / (ranges[j][1] - ranges[j][0]))
    vals = list(overlap.values())
    if any(near(a, b) for p, a in enumerate(vals) for b in vals[p + 1:]) or any(near(a, alpha) for a in vals):
        return "two overlaps, or an overlap and alpha, are nearly equal"
    align_orders, steps = R.schedule(ranges, mutual_nn, overlap, alpha, f["realign_panorama"])
    assert align_orders == e["align_orders"] and list(overlap.items()) == list(e["overlap"].items())
    for key, pairs in mutual_nn.items():
        assert np.array_equal(R.pairs_array(pairs), e["mutual_nn"][key])
        out["%s_mnn_%d_%d" % (name, key[0], key[1])] = R.pairs_array(pairs)
    out[name + "_overlap"] = np.array(vals)
    out[name + "_orders"] = np.array(align_orders, dtype=np.int32).reshape(-1, 2)
    out[name + "_steps"] = np.array([(len(s["cur_rows"]), len(s["mnn_cur"])) for s in steps], dtype=np.int64).reshape(-1, 2)
    # the chains: the reference's in f64 from its own correction_vector, the exact one in longdouble
    x_ref, x_exact = np.array(x), np.array(x, dtype=LD)
    score_before = ref.batch_effect_score(x_ref, ids, max_num_bcs=f["max_num_bcs"])
    exact_corr, worst = [], 0.0
    for s, st in enumerate(steps):
        ref_corr = ref.correction_vector(x_ref, st["cur_rows"], list(st["mnn_cur"]), list(st["mnn_ref"]), sigma)
        same_state = R.correction(x_ref, st["cur_rows"], st["mnn_cur"], st["mnn_ref"], sigma, LD)
        dev = R.rel_dev(ref_corr, same_state)
        worst = max(worst, dev)
        assert dev <= 1e-9, "%s step %d: scikit-learn's correction_vector is %.3g from exact" % (name, s, dev)
        assert np.array_equal(np.isnan(ref_corr), np.isnan(np.asarray(same_state, dtype=np.float64)))
        corr, den = R.correction(x_exact, st["cur_rows"], st["mnn_cur"], st["mnn_ref"], sigma, LD, want_den=True)
        if ((den > 0) & (den < 1e-250)).any():
            return "a row's den lies in (0, 1e-250)"
        rows = sample(len(st["cur_rows"]), CORR_ROWS, 1000 + s)
        out["%s_corr%d_rows" % (name, s)] = rows.astype(np.int32)
        out["%s_corr%d_ref" % (name, s)] = ref_corr[rows]
        out["%s_corr%d_hi" % (name, s)], out["%s_corr%d_lo" % (name, s)] = hi_lo(corr[rows])
        out["%s_corr%d_scale" % (name, s)] = np.float64(R.max_abs(corr))
        x_ref[st["cur_rows"]] += ref_corr
        x_exact[st["cur_rows"]] += corr
        exact_corr.append(corr)
    if min(score_gap(x, ids, f["max_num_bcs"]), score_gap(x_ref, ids, f["max_num_bcs"]), score_gap(e["final"], ids, f["max_num_bcs"])) < 1e-9:
        return "a score query's d2 gap at the k boundary is below 1e-9"
    score_after = ref.batch_effect_score(x_ref, ids, max_num_bcs=f["max_num_bcs"])
    assert score_before == e["score_before"], "%s: the restatement's score before differs from the reference's" % name
    rows = sample(len(x), FINAL_ROWS, 7)
    out[name + "_final_rows"] = rows.astype(np.int32)
    out[name + "_final_ref"] = x_ref[rows]
    out[name + "_final_hi"], out[name + "_final_lo"] = hi_lo(x_exact[rows])
    out[name + "_final_scale"] = np.float64(R.max_abs(x_exact))
    out[name + "_score_before"], out[name + "_score_after"] = np.float64(score_before), np.float64(score_after)
    # the restatement's deviation from exact over three pair orders
    dev_corr, dev_final = 0.0, 0.0
    for order_name, permute in R.PAIR_ORDERS.items():
        final, corrs = R.run_steps(x, steps, sigma, np.float64, permute)
        dev_final = max(dev_final, R.rel_dev(final, x_exact))
        for got, exact in zip(corrs, exact_corr):
            dev_corr = max(dev_corr, R.rel_dev(got, exact))
    dev_corr, dev_final = max(dev_corr, ROUNDING), max(dev_final, ROUNDING)
    out[name + "_dev_corr"], out[name + "_dev_final"] = np.float64(dev_corr), np.float64(dev_final)
    print("%-16s steps %d, scikit-learn from exact %.3g, restatement from exact: corr %.3g, final %.3g; scores %.6f -> %.6f"
          % (name, len(steps), worst, dev_corr, dev_final, score_before, score_after))
    return None


def correction_fixture(name, f, ref, out):
    args = (f["x"], f["cur_rows"], f["mnn_cur"], f["mnn_ref"], f["sigma"])
    exact, den = R.correction(*args, dtype=LD, want_den=True)
    if ((den > 0) & (den < 1e-250)).any():
        return "a row's den lies in (0, 1e-250)"
    with np.errstate(invalid="ignore", divide="ignore"):
        ref_corr = ref.correction_vector(f["x"], f["cur_rows"], list(f["mnn_cur"]), list(f["mnn_ref"]), f["sigma"])
    dev_ref = R.rel_dev(ref_corr, exact)
    assert dev_ref <= 1e-9, "%s: scikit-learn's correction_vector is %.3g from exact" % (name, dev_ref)
    assert np.array_equal(np.isnan(ref_corr), np.isnan(np.asarray(exact, dtype=np.float64))), "%s: the NaN rows differ" % name
    dev = 0.0
    for order_name, permute in R.PAIR_ORDERS.items():
        order = np.arange(len(f["mnn_cur"])) if permute is None else permute(0, len(f["mnn_cur"]))
        got = R.correction(f["x"], f["cur_rows"], f["mnn_cur"][order], f["mnn_ref"][order], f["sigma"])
        assert np.array_equal(np.isnan(got), np.isnan(ref_corr))
        dev = max(dev, R.rel_dev(got, exact))
    out[name + "_ref"] = ref_corr
    out[name + "_hi"], out[name + "_lo"] = hi_lo(exact)
    dev = max(dev, ROUNDING)
    out[name + "_dev"] = np.float64(dev)
    print("%-16s scikit-learn from exact %.3g, restatement from exact %.3g, NaN rows %d" % (name, dev_ref, dev, int(np.isnan(ref_corr).any(axis=1).sum())))
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="a checkout of the reference (its lib/python is imported)")
    a = ap.parse_args()
    import sklearn

    assert sklearn.__version__ == "1.7.2", "the reference is scikit-learn 1.7.2, this is %s" % sklearn.__version__
    sys.path.insert(0, os.path.join(a.reference, "lib", "python"))
    import cellranger.analysis.batch_correction as ref

    out, rejected, total = {}, [], 0
    for name, f in R.FIXTURES.items():
        total += 1
        part = {}
        why = stage_fixture(name, f, ref, part)
        if why:
            rejected.append((name, why))
        else:
            out.update(part)
    for name, f in R.CORRECTIONS.items():
        total += 1
        part = {}
        why = correction_fixture(name, f, ref, part)
        if why:
            rejected.append((name, why))
        else:
            out.update(part)
    print("fixtures: %d, rejected: %d %s" % (total, len(rejected), rejected))
    if 8 * len(rejected) > total:
        raise SystemExit("more than 1 fixture in 8 rejected")
    if rejected:
        raise SystemExit("change the seed of %s in tests/batch_correction_numpy.py" % [n for n, _ in rejected])
    np.savez_compressed(OUT, **out)
    print("%s: %d bytes" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
