"""Records tests/golden/sseq_reference.npz: for every fixture of tests/sseq_numpy.py the restatement's outputs, and every p-value and
adjusted p-value in exact arithmetic (mpmath, 40 digits, from the integer matrix on -- the parameters too, so that the exact values do
not inherit a rounding of the restatement's parameters).

A fixture is rejected, named, and replaced by its next seed when a comparison would hang on a rounding: some exact-test term with
0 < |l_i - l_obs| < 1e-6, an asymptotic test with |(x_a + 0.5) / T - median| < 1e-9, or a count sum of exactly 900 outside the fixture
that constructs them.  At most one fixture in eight may be rejected; the count is printed and stored.

dev_<q> = the largest deviation of the restatement from the exact value over all fixtures (exact_p, asymptotic_p, adjusted_p: relative),
or, for the parameters and means, which are sums over cells without an exact twin in the file, the largest movement between three
orders of those sums (relative; log2_fold_change against max(1, |value|)).  The GPU test allows 16 x dev_<q>.

    python scripts/make_sseq_golden.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sseq_numpy as R  # noqa: E402

PARAM_KEYS = ("size_factors", "mean_g", "var_g", "use_g", "phi_mm_g", "phi_g", "zeta_hat", "delta", "n_used")
OUT_KEYS = ("sums_in", "sums_out", "norm_mean_in", "norm_mean_out", "log2_fold_change", "p_values", "adjusted_p_values", "below_median", "s_a", "s_b",
            "n_exact", "n_asymptotic")
MOVING = dict(mean_g="mean_g", var_g="var_g", phi_mm_g="phi_g", phi_g="phi_g", zeta_hat="zeta_hat", delta="delta", norm_mean_in="norm_mean",
              norm_mean_out="norm_mean", s_a="norm_mean", s_b="norm_mean", log2_fold_change="log2_fold_change")


def err(got, ref, floor=0.0):
    """the largest |got - ref| / max(|ref|, floor) over the finite entries of ref that are not 0 (0 must be met exactly)"""
    got, ref = np.atleast_1d(np.asarray(got, np.float64)), np.atleast_1d(np.asarray(ref, np.float64))
    ok = np.isfinite(ref) & ((ref != 0) | (floor > 0))
    if not ok.any():
        return 0.0
    return float(np.max(np.abs(got[ok] - ref[ok]) / np.maximum(np.abs(ref[ok]), floor)))


def why_rejected(name, x, P, o):
    if np.any(o["min_gap"] < 1e-6):
        return "an exact-test term %.3g from the observed one" % o["min_gap"].min()
    big = o["below_median"] != 255
    T = (o["sums_in"] + o["sums_out"]).astype(np.float64)
    if big.any() and np.min(np.abs((o["sums_in"][big] + 0.5) / T[big] - o["median"][big])) < 1e-9:
        return "an asymptotic test on the median"
    use = P["use_g"]
    if name not in R.CONSTRUCTED_900 and (np.any(o["sums_in"][:, use] == R.BIG_COUNT) or np.any(o["sums_out"][:, use] == R.BIG_COUNT)):
        return "a count sum of exactly %d" % R.BIG_COUNT
    return None


def main():
    out, dev, rejected = {}, {}, []
    for name in sorted(R.FIXTURES):
        bump = 0
        while True:
            x, labels, K = R.fixture(name, bump)
            P = R.compute_params(x)
            o = R.diffexp(x, P, labels, K)
            why = why_rejected(name, x, P, o)
            if why is None:
                break
            print("rejected: %s (seed bump %d): %s" % (name, bump, why))
            rejected.append("%s+%d" % (name, bump))
            bump += 1
        assert len(rejected) * 8 <= len(R.FIXTURES), "more than one fixture in eight rejected"
        mp_p, mp_adj, _, _ = R.diffexp_mp(x, labels, K)
        out[name + "/bump"], out[name + "/x_sum"], out[name + "/labels"] = bump, int(x.sum()), labels
        for k in PARAM_KEYS:
            out["%s/%s" % (name, k)] = P[k]
        for k in OUT_KEYS:
            out["%s/%s" % (name, k)] = o[k]
        out[name + "/mp_p"], out[name + "/mp_adj"] = mp_p, mp_adj
        big, use = o["below_median"] != 255, P["use_g"]
        exact = ~big & use[None, :]
        d = dict(exact_p=err(o["p_values"][exact], mp_p[exact]), asymptotic_p=err(o["p_values"][big], mp_p[big]) if big.any() else 0.0,
                 adjusted_p=err(o["adjusted_p_values"], mp_adj))
        for order in (1, 2):      # how far the sums over cells move the parameters and the means
            P2 = R.compute_params(x, order)
            o2 = R.diffexp(x, P2, labels, K, order, want_p=False)
            for k, q in MOVING.items():
                src, src2 = (P, P2) if k in P else (o, o2)
                d[q] = max(d.get(q, 0.0), err(src2[k], src[k], 1.0 if q == "log2_fold_change" else 0.0))
        print("%-22s G %3d N %3d K %2d  used %3d  exact %4d  asymptotic %3d  longest %6d terms  %s" % (
            name, x.shape[0], x.shape[1], K, P["n_used"], int(o["n_exact"].sum()), int(o["n_asymptotic"].sum()),
            int((o["sums_in"] + o["sums_out"])[exact].max()) + 1 if exact.any() else 0, "  ".join("%s %.2e" % kv for kv in sorted(d.items()))))
        for q, v in d.items():
            dev[q] = max(dev.get(q, 0.0), v)
    for q, v in sorted(dev.items()):
        out["dev_" + q] = v
        print("dev_%-18s %.3e" % (q, v))
    out["n_rejected"], out["rejected"] = len(rejected), np.array(rejected, dtype="U40")
    print("fixtures rejected: %d %s" % (len(rejected), rejected))
    path = os.path.join(ROOT, "tests", "golden", "sseq_reference.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
