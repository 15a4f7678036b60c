#!/usr/bin/env python
"""Record tests/golden/umap_reference.npz from tests/umap_numpy.py and scipy 1.15.3 (CPU only).

Per fixture <name>_rho, _sigma, _steps, _indptr, _indices, _values: the restatement's fuzzy graph after the prune.  A fixture is REJECTED
when any step of any row's search has |psum - log2(k + 1)| within 1e-9 of the tolerance 1e-5 (the one comparison a step that ends
the search makes; a step that goes on also compares psum with the target, from which it is then 1e-5 away), or when an entry of the
union lies within 1e-9 relative of the prune threshold wmax / n_epochs: there a last bit of exp could turn a decision, elsewhere the
device's rho, steps and CSR structure are expected to be bit-equal ("k of n rejected" is printed; change the seed of a rejected
fixture in tests/umap_numpy.py).

ab_cases [4, 2] = (min_dist, spread); ab_scipy [4, 2] = scipy.optimize.curve_fit of 1 / (1 + a x^(2b)) on umap-learn's 300 points from
the start (1, 1) at ftol = xtol = gtol = 1e-14; ab_bound [4, 2] = 16 times the distance to scipy's answer from the start (2, 0.5),
floored at 1e-12 relative.

three_groups_apart: the three groups are apart in the restatement's embedding for the seeds 0, 1, 2 (all epochs), and
three_groups_largest_move the largest per-epoch move of a coordinate among them.

    python scripts/make_umap_golden.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import umap_numpy as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "umap_reference.npz")
NEAR = 1e-9


def groups_apart(Y, size=100):
    """every row nearer to its own group's mean than to another's"""
    means = np.stack([Y[g * size:(g + 1) * size].mean(axis=0) for g in range(len(Y) // size)])
    near = np.argmin(((Y[:, None, :] - means[None]) ** 2).sum(axis=2), axis=1)
    return bool((near == np.repeat(np.arange(len(means)), size)).all())


def near_a_decision(g):
    h = np.abs(g["decisions"])
    search = bool((np.abs(h - R.TOL) < NEAR).any())
    prune = bool((np.abs(g["union_values"] - g["threshold"]) < NEAR * g["threshold"]).any())
    return search, prune


def main():
    import scipy
    from scipy.optimize import curve_fit

    assert scipy.__version__ == "1.15.3", "the reference is scipy 1.15.3, this is %s" % scipy.__version__
    out, rejected = {}, []
    for name in R.FIXTURES:
        g = R.prepared(name)
        search, prune = near_a_decision(g)
        if search or prune:
            rejected.append(name)
            print("REJECTED %s: %s" % (name, "a search step near a decision" if search else "an entry near the prune threshold"))
            continue
        for key in ("rho", "sigma", "steps", "indptr", "indices", "values"):
            out["%s_%s" % (name, key)] = g[key]
        print("%-14s n %4d k %3d nnz %6d of %6d, steps up to %2d, %d rows at the floor, %d rows with rho 0" % (
            name, len(g["rho"]), g["k"], g["nnz"], len(g["union_values"]), g["steps"].max(), g["floored"].sum(), (g["rho"] == 0).sum()))
    print("%d of %d rejected" % (len(rejected), len(R.FIXTURES)))
    if rejected:
        sys.exit(1)

    def f(x, a, b):
        return 1.0 / (1.0 + a * x ** (2 * b))

    fits, bounds = [], []
    for min_dist, spread in R.AB_CASES:
        x, y = R.curve(min_dist, spread)
        r = [curve_fit(f, x, y, p0=p0, ftol=1e-14, xtol=1e-14, gtol=1e-14)[0] for p0 in ((1.0, 1.0), (2.0, 0.5))]
        fits.append(r[0])
        bounds.append(np.maximum(16.0 * np.abs(r[0] - r[1]), 1e-12 * np.abs(r[0])))
        mine = np.array(R.umap_ab(min_dist, spread))
        print("min_dist %-5g spread %g: scipy a %.12f b %.12f, the restatement off by %.3g, %.3g of the bound" % (
            min_dist, spread, r[0][0], r[0][1], *(np.abs(mine - r[0]) / bounds[-1])))
        assert (np.abs(mine - r[0]) <= bounds[-1]).all()
    out.update(ab_cases=np.array(R.AB_CASES), ab_scipy=np.array(fits), ab_bound=np.array(bounds))

    g, fx = R.prepared("three_groups"), R.FIXTURES["three_groups"]
    a, b = R.umap_ab()
    apart, move = [], 0.0
    for seed in (0, 1, 2):
        Y, _, _, totals, _ = R.run(g["indptr"], g["indices"], g["values"], g["y0"], 0, fx.n_epochs, fx.n_epochs, a, b, seed)
        apart.append(groups_apart(Y) and bool(np.isfinite(Y).all()))
        move = max(move, totals["largest_move"])
        print("three_groups seed %d: apart %s, largest per-epoch move %.2f, n_neg up to %d" % (seed, apart[-1], totals["largest_move"], totals["max_n_neg"]))
    assert all(apart)
    out.update(three_groups_apart=np.array(apart), three_groups_largest_move=np.float64(move))
    np.savez_compressed(OUT, **out)
    print("wrote %s: %d bytes" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
