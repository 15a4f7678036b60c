#!/usr/bin/env python
"""Record tests/golden/tsne_reference.npz from tests/tsne_numpy.py and scikit-learn 1.7.2 (CPU only).

Per fixture <name>_beta, _steps, _indptr, _indices, _values: the restatement's search and symmetrised P.  A fixture is REJECTED when
any step of any row's search has |H - log(perplexity)| within 1e-9 of the tolerance 1e-5 or of 0: there a last bit of exp could turn
a decision, elsewhere the device's beta and step counts are expected to be bit-equal ("k of n rejected" is printed; change the seed
of a rejected fixture in tests/tsne_numpy.py).

Per fixture of tsne_numpy.SKLEARN_FIXTURES <name>_Y [3, n, dims] (the start, after stop_lying_iter and after max_iter iterations of the
restatement under tsne_numpy.TRAJECTORY's settings), <name>_grad = sklearn.manifold._t_sne._kl_divergence's gradient / 4 and <name>_kl
its cost at each of them on the dense P, and <name>_grad_bound, <name>_kl_bound [3]: 16 times the restatement's own movement between
three candidate orders (chunks of 4096, 64 and 7), floored at one rounding of the largest magnitude.  The restatement must lie within
them, or the maker stops.

three_groups_final_kl, three_groups_kl_margin: the restatement's cost after the stage's 1000 iterations and 16 times the spread of that
cost when every value of P is moved by one ulp up or down at random, three times (the descent amplifies a last bit; the margin says by
how much).  three_groups_kmeans_ok: the three groups are apart in the restatement's embedding.

    python scripts/make_tsne_golden.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import tsne_numpy as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "tsne_reference.npz")
NEAR = 1e-9
EPS = 2.0 ** -53


def dense(a, n):
    P = np.zeros((n, n))
    rows = np.repeat(np.arange(n), np.diff(a["indptr"]))
    P[rows, a["indices"]] = a["values"]
    return P


def groups_apart(Y, size=100):
    """every row nearer to its own group's mean than to another's"""
    means = np.stack([Y[g * size:(g + 1) * size].mean(axis=0) for g in range(len(Y) // size)])
    near = np.argmin(((Y[:, None, :] - means[None]) ** 2).sum(axis=2), axis=1)
    return bool((near == np.repeat(np.arange(len(means)), size)).all())


def main():
    import sklearn
    from scipy.spatial.distance import squareform
    from sklearn.manifold import _t_sne

    assert sklearn.__version__ == "1.7.2", "the reference is scikit-learn 1.7.2, this is %s" % sklearn.__version__
    out, rejected = {}, []
    for name in R.FIXTURES:
        a = R.prepared(name)
        h = np.abs(a["hdiff"][np.isfinite(a["hdiff"])])
        if ((np.abs(h - R.TOL) < NEAR) | (h < NEAR)).any():
            rejected.append(name)
            continue
        for key in ("beta", "steps", "indptr", "indices", "values"):
            out["%s_%s" % (name, key)] = a[key]
        print("%-16s n = %3d, k = %3d, nnz = %5d, at most %3d steps, total %.17g" % (name, len(a["x"]), a["k"], len(a["values"]), a["steps"].max(),
                                                                                      a["p_total"]))
    print("%d of %d rejected %s" % (len(rejected), len(R.FIXTURES), rejected))
    if rejected:
        raise SystemExit("change the seed of %s in tests/tsne_numpy.py" % rejected)

    T = R.TRAJECTORY
    for name in R.SKLEARN_FIXTURES:
        a, f = R.prepared(name), R.FIXTURES[name]
        n = len(a["x"])
        csr = (a["indptr"], a["indices"], a["values"])
        Y1, uY, gains, _ = R.run(*csr, a["y0"], 0, T["stop_lying_iter"], T["stop_lying_iter"], T["mom_switch_iter"])
        Y2 = R.run(*csr, Y1, T["stop_lying_iter"], T["max_iter"] - T["stop_lying_iter"], T["stop_lying_iter"], T["mom_switch_iter"], uY, gains)[0]
        Ys = np.stack([a["y0"], Y1, Y2])
        P = squareform(dense(a, n), checks=True)
        grads, kls, gb, kb = [], [], [], []
        for Y in Ys:
            kl, g = _t_sne._kl_divergence(Y.ravel().copy(), P, 1.0, n, f.dims)
            g = g.reshape(n, f.dims) / 4.0
            mine = [R.gradient(*csr, Y, 1.0, chunk) for chunk in (R.CAND_CHUNK, 64, 7)]
            mine_kl = [R.cost(*csr, Y, Z) for _, Z in mine]
            g_bound = 16.0 * max(max(np.abs(m[0] - mine[0][0]).max() for m in mine), EPS * np.abs(g).max())
            k_bound = 16.0 * max(max(abs(k - mine_kl[0]) for k in mine_kl), EPS * abs(kl))
            dev_g, dev_k = np.abs(mine[0][0] - g).max(), abs(mine_kl[0] - kl)
            print("%-16s |grad| <= %.3g: restatement - sklearn / 4 = %.3g (bound %.3g); kl = %.6f: difference %.3g (bound %.3g)" % (
                name, np.abs(g).max(), dev_g, g_bound, kl, dev_k, k_bound))
            if dev_g > g_bound or dev_k > k_bound:
                raise SystemExit("%s: the restatement leaves scikit-learn's gradient or cost" % name)
            grads.append(g), kls.append(kl), gb.append(g_bound), kb.append(k_bound)
        out[name + "_Y"], out[name + "_grad"], out[name + "_kl"] = Ys, np.stack(grads), np.array(kls)
        out[name + "_grad_bound"], out[name + "_kl_bound"] = np.array(gb), np.array(kb)

    a = R.prepared("three_groups")
    finals = []
    rs = np.random.RandomState(20261026)
    for trial in range(4):
        v = a["values"] if trial == 0 else np.nextafter(a["values"], np.where(rs.randint(0, 2, len(a["values"])) == 1, np.inf, -np.inf))
        Y = R.run(a["indptr"], a["indices"], v, a["y0"], 0, 1000, 250, 250)[0]
        finals.append(R.cost(a["indptr"], a["indices"], v, Y))
        if trial == 0:
            out["three_groups_kmeans_ok"] = np.array(groups_apart(Y))
            assert out["three_groups_kmeans_ok"], "the three groups are not apart in the restatement's embedding"
    out["three_groups_final_kl"] = np.array(finals[0])
    out["three_groups_kl_margin"] = np.array(16.0 * (max(finals) - min(finals)))
    print("three_groups: final kl %s, margin %.3g" % (["%.9f" % k for k in finals], float(out["three_groups_kl_margin"])))
    np.savez_compressed(OUT, **out)
    print("%s: %d bytes" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
