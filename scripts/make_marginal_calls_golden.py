#!/usr/bin/env python
"""Record the reference's own marginal calls for a set of fixture rows -> tests/golden/marginal_calls_reference.npz.

    python scripts/make_marginal_calls_golden.py <reference checkout>/lib/python

Runs on the CPU.  At record time it loads call_presence_with_gmm_ab and TagAssigner.identify_contaminant_tags from the reference's
cellranger.feature.feature_assigner on the given path; the imports of that module that are not installed here (the HDF5 matrix
classes, tenkit, ...) are stubbed, the two functions need none of them.  Nothing of the reference is copied: the file holds the
fixture rows (built here), what the reference returned for them, and what scikit-learn's fitted object reported.

Per fixture row: V, the sparse row (columns, counts), umi_threshold, the reference's calls, and from an identical GaussianMixture fit
the weights / means / covariance / n_iter_ / lower_bound_ (the reference function keeps only the calls; the parameters come from the
same constructor arguments on the same data, and its calls are checked against the reference's here).
Also: the scikit-learn version; the 30 doubles and the order in which scikit-learn draws them (recorded from a RandomState that logs
its calls: per init one choice(n, p) -- one double -- and one uniform(size=2)); the contaminant outcome of one 12-tag fixture;
`movement`: max |reference - restatement in cell order| and max |cell order - histogram order| over the fixtures, separately for
weights, means and covariance, all absolute.

A candidate fixture row is REJECTED (and the next seed tried), so that integers and iteration counts can be asserted equal:
  * in the restatement any init's stopping difference | |change| - 1e-3 | is below 1e-9;
  * a Lloyd midpoint or the winner's decision boundary lies within 1e-9 of a data value (of log10(1 + count)); a row of one
    distinct value over all cells is exempt from the midpoint half (its centres are that value by construction)."""
import os
import sys
import types
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import marginal_calls_numpy as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "marginal_calls_reference.npz")
MARGIN = 1e-9


class _Anything:
    """stands for whatever a stubbed module is asked for"""

    def __init__(self, *a, **k):
        pass

    def __call__(self, *a, **k):
        return _Anything()

    def __getattr__(self, name):
        return _Anything()

    def __mro_entries__(self, bases):
        return (object,)


class _Stub(types.ModuleType):
    __path__ = []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return _Anything()


def load_reference(ref_path):
    """cellranger.feature.feature_assigner with every cellranger / tenkit module it imports stubbed (they need HDF5 and an older
    numpy; the two functions recorded here use numpy, pandas and scikit-learn only), and any other module that is not installed"""
    import ast

    sys.path.insert(0, ref_path)
    with open(os.path.join(ref_path, "cellranger", "feature", "feature_assigner.py")) as f:
        tree = ast.parse(f.read())
    wanted = set()
    for node in tree.body:
        if isinstance(node, ast.Import):
            wanted.update(a.name for a in node.names)
        elif isinstance(node, ast.ImportFrom) and node.module:
            wanted.add(node.module)
    for name in sorted(wanted):
        if name.split(".")[0] not in ("cellranger", "tenkit"):
            continue
        parts = name.split(".")
        for d in range(1, len(parts) + 1):
            sub = ".".join(parts[:d])
            if sub in ("cellranger", "cellranger.feature") or sub in sys.modules:
                continue
            sys.modules[sub] = _Stub(sub)
            if d > 1 and ".".join(parts[:d - 1]) in sys.modules:
                setattr(sys.modules[".".join(parts[:d - 1])], parts[d - 1], sys.modules[sub])
    for _ in range(50):
        try:
            import cellranger.feature.feature_assigner as fa

            return fa
        except ImportError as e:      # a third-party module that is not installed: stub it and try again
            if not e.name or e.name in sys.modules:
                raise
            sys.modules[e.name] = _Stub(e.name)
    raise RuntimeError("the reference module does not load")


class LoggingRandomState(np.random.RandomState):
    """logs which methods scikit-learn calls, in order, and the doubles they consume"""

    def __init__(self, seed):
        super().__init__(seed)
        self.log = []

    def choice(self, a, size=None, replace=True, p=None):
        before = self.get_state()
        out = super().choice(a, size=size, replace=replace, p=p)
        probe = np.random.RandomState()
        probe.set_state(before)
        self.log.append(("choice", [probe.random_sample()]))
        assert probe.get_state()[2] == self.get_state()[2] and np.array_equal(probe.get_state()[1], self.get_state()[1]), "choice() took more than one double"
        return out

    def uniform(self, low=0.0, high=1.0, size=None):
        out = super().uniform(low, high, size)
        self.log.append(("uniform", list(np.ravel(out))))
        return out


def sklearn_fit(counts, random_state=0):
    from sklearn import mixture

    x = np.log10(1 + counts).reshape(-1, 1)
    g = mixture.GaussianMixture(n_components=2, n_init=10, covariance_type="tied", random_state=random_state)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        g.fit(x)
        pred = g.predict(x)
    return g, pred


def fixture_rows():
    """-> list of (name, V, umi_threshold, generator(rng) -> counts i64[V])"""
    def guide(V, frac, bg=0.02):
        def f(rng):
            c = rng.poisson(bg, V)
            k = rng.random(V) < frac
            c[k] += rng.negative_binomial(3, 0.05, k.sum())
            return c
        return f

    def antibody(V, spread):
        def f(rng):
            c = rng.negative_binomial(2, spread, V)
            k = rng.random(V) < 0.3
            c[k] = c[k] * 20 + 50
            return c
        return f

    def tag(V, frac):
        def f(rng):
            c = rng.poisson(3.0, V)
            k = rng.random(V) < frac
            c[k] += rng.poisson(400, k.sum())
            return c
        return f

    def const(V, v, frac):
        return lambda rng: np.where(rng.random(V) < frac, v, 0)

    def one_entry(V, v):
        def f(rng):
            c = np.zeros(V, np.int64)
            c[rng.integers(V)] = v
            return c
        return f

    rows = [("v2_a", 2, 1, lambda rng: np.array([0, 3])), ("v2_b", 2, 1, lambda rng: np.array([2, 2])), ("v2_c", 2, 3, lambda rng: np.array([1, 5])),
            ("v2_zero", 2, 1, lambda rng: np.array([0, 0])),
            ("v3_a", 3, 1, lambda rng: np.array([0, 0, 4])), ("v3_b", 3, 1, lambda rng: np.array([1, 2, 3])), ("v3_c", 3, 3, lambda rng: np.array([5, 5, 5])),
            ("v3_d", 3, 1, lambda rng: np.array([0, 7, 0]))]
    for V in (65, 257):
        rows += [("v%d_guide" % V, V, 3, guide(V, 0.15)), ("v%d_guide_lo" % V, V, 3, guide(V, 0.05, 0.2)), ("v%d_tag" % V, V, 1, tag(V, 0.2)),
                 ("v%d_antibody" % V, V, 1, antibody(V, 0.02)), ("v%d_one_value" % V, V, 1, const(V, 6, 0.3)), ("v%d_one_value_full" % V, V, 3, const(V, 9, 1.1)),
                 ("v%d_one_entry" % V, V, 1, one_entry(V, 12)), ("v%d_zero" % V, V, 1, const(V, 0, 0.5)), ("v%d_no_zeros" % V, V, 1, lambda rng, V=V: 1 + rng.poisson(4.0, V)),
                 ("v%d_guide_b" % V, V, 3, guide(V, 0.3)), ("v%d_tag_b" % V, V, 1, tag(V, 0.5))]
    V = 5000
    rows += [("v5000_guide_%d" % i, V, 3, guide(V, f)) for i, f in enumerate((0.01, 0.03, 0.1))]
    rows += [("v5000_tag_%d" % i, V, 1, tag(V, f)) for i, f in enumerate((0.08, 0.25))]
    rows += [("v5000_antibody_64", V, 1, antibody(V, 0.05)), ("v5000_antibody_256", V, 1, antibody(V, 0.004)), ("v5000_one_value", V, 3, const(V, 4, 0.02)),
             ("v5000_one_entry", V, 1, one_entry(V, 30)), ("v5000_no_zeros", V, 1, lambda rng: 1 + rng.negative_binomial(2, 0.01, V))]
    return rows


def params_of(g):
    mu = g.means_.ravel()
    hi = int(np.argmax(mu))
    lo = 1 - hi
    return np.array([g.weights_[lo], g.weights_[hi]]), np.array([mu[lo], mu[hi]]), float(g.covariances_.ravel()[0])


def params_of_res(r):
    return np.array([r["weight_low"], r["weight_high"]]), np.array([r["mean_low"], r["mean_high"]]), float(r["covariance"])


def contaminant_fixture(fa):
    """12 tags on 400 cells: a dominant set, a weak tag (< 1000), a tag 50-fold below the top, a zero tag, a correlated pair, a constant one"""
    rng = np.random.default_rng(77)
    V, k = 400, 12
    counts = np.zeros((k, V), np.int64)
    owner = rng.integers(0, 8, V)
    for t in range(8):
        counts[t] = rng.poisson(2.0, V) + np.where(owner == t, rng.poisson(3000, V), 0)
    counts[8] = rng.poisson(0.5, V)                                   # fewer than 1000 UMIs
    counts[9] = 0                                                     # no UMI: dropped
    counts[10] = counts[2] // 3 + rng.poisson(1.0, V)                 # follows tag 2 with fewer UMIs
    counts[11] = 500                                                  # constant: its correlations are NaN
    counts[3] = np.where(owner == 3, rng.poisson(40, V), 0) + rng.poisson(0.2, V)   # >= 1000 UMIs, but 50-fold below the top
    ids = [b"CMO%03d" % ((7 * t + 3) % 12) for t in range(k)]         # the sorted-id order is not the row order
    order = np.argsort(np.array(ids)).astype(np.uint32)

    class Defs:
        def __init__(self, i):
            self.id = i

    class Sub:
        bcs = [b"BC%04d" % i for i in range(V)]

        class feature_ref:
            feature_defs = [Defs(i) for i in ids]

        class m:
            @staticmethod
            def toarray():
                return counts

    class Self:
        feature_type = "Multiplexing Capture"

        class matrix:
            @staticmethod
            def select_features_by_type(_):
                return Sub

    assts = {ids[t]: fa.FeatureAssignments(np.zeros(0, np.int64), int(counts[t].sum()), False, []) for t in range(k)}
    out = fa.TagAssigner.identify_contaminant_tags(Self(), assts)
    flags = np.full(k, 2, np.uint8)
    sources = np.full((k, k), -1, np.int32)
    for t in range(k):
        if ids[t] in out:
            flags[t] = 1 if out[ids[t]].is_contaminant else 0
            for s, other in enumerate(out[ids[t]].correlated_features):
                sources[t, s] = ids.index(other)
    return counts, order, flags, sources


def main(ref_path):
    import sklearn

    assert sklearn.__version__ == R.SKLEARN_VERSION, "the restatement follows scikit-learn %s" % R.SKLEARN_VERSION
    fa = load_reference(ref_path)
    # ---- the consumption pattern of the random stream ----
    rs = LoggingRandomState(0)
    sklearn_fit(np.random.default_rng(1).poisson(1.0, 300), rs)
    assert [k for k, _ in rs.log] == ["choice", "uniform"] * 10 and all(len(v) == (1 if k == "choice" else 2) for k, v in rs.log), rs.log
    drawn = np.array([x for _, v in rs.log for x in v])
    u300, _ = R.seed_draws(300)
    assert drawn.tobytes() == u300.ravel().tobytes(), "the 30 doubles are not RandomState(0)'s first 30"
    after = np.random.RandomState(0)
    after.random_sample(30)
    assert rs.get_state()[2] == after.get_state()[2] and np.array_equal(rs.get_state()[1], after.get_state()[1]), "the fit drew more than the 30 logged doubles"
    out = dict(sklearn_version=np.array(sklearn.__version__), draws=drawn, draw_order=np.array(["choice", "uniform", "uniform"] * 10))
    # ---- the fixture rows ----
    move = dict(ref_w=0.0, ref_mu=0.0, ref_cov=0.0, form_w=0.0, form_mu=0.0, form_cov=0.0)
    names, Vs, thrs, ptr, cols_all, vals_all, call_ptr, calls_all = [], [], [], [0], [], [], [0], []
    par = dict(w=[], mu=[], cov=[], n_iter=[], lb=[], fitted=[], seed=[])
    landings, first_kinds = np.zeros(4, np.int64), np.zeros(2, np.int64)
    for ri, (name, V, thr, gen) in enumerate(fixture_rows()):
        for attempt in range(50):
            seed = 1000 * ri + attempt
            counts = np.asarray(gen(np.random.default_rng(seed)), np.int64)
            assert len(counts) == V
            ref_calls = np.asarray(fa.call_presence_with_gmm_ab(counts, umi_threshold=thr), bool)
            cols = np.flatnonzero(counts)
            dense = R.fit_dense(counts, thr)
            hist = R.fit_histogram(V, cols, counts[cols], thr)
            if not dense["fitted"]:
                assert not ref_calls.any() and not hist["fitted"]
                break
            xs = np.unique(np.log10(1 + counts))
            if R.margins_ok(dense, xs, MARGIN) and R.margins_ok(hist, xs, MARGIN):
                break
            print("rejected", name, "seed", seed)
        else:
            raise RuntimeError("no acceptable fixture for " + name)
        names.append(name), Vs.append(V), thrs.append(thr)
        cols_all.append(cols), vals_all.append(counts[cols]), ptr.append(ptr[-1] + len(cols))
        on = np.flatnonzero(ref_calls)
        calls_all.append(on), call_ptr.append(call_ptr[-1] + len(on))
        par["fitted"].append(bool(dense["fitted"])), par["seed"].append(seed)
        if not dense["fitted"]:
            par["w"].append([np.nan] * 2), par["mu"].append([np.nan] * 2), par["cov"].append(np.nan), par["n_iter"].append(0), par["lb"].append(np.nan)
            continue
        g, pred = sklearn_fit(counts)
        assert np.array_equal(ref_calls, (counts >= thr) & (pred == np.argmax(g.means_))), name
        w, mu, cov = params_of(g)
        par["w"].append(w), par["mu"].append(mu), par["cov"].append(cov), par["n_iter"].append(int(g.n_iter_)), par["lb"].append(float(g.lower_bound_))
        hc = np.zeros(V, bool)
        hc[cols] = hist["calls"]
        assert np.array_equal(ref_calls, dense["calls"]) and np.array_equal(ref_calls, hc), name
        assert dense["n_iter"] == hist["n_iter"] == g.n_iter_ and dense["winner"] == hist["winner"], (name, dense["n_iter"], hist["n_iter"], g.n_iter_)
        dw, dmu, dcov = params_of_res(dense)
        hw, hmu, hcov = params_of_res(hist)
        for key, a, b in (("ref_w", w, dw), ("ref_mu", mu, dmu), ("ref_cov", cov, dcov), ("form_w", hw, dw), ("form_mu", hmu, dmu), ("form_cov", hcov, dcov)):
            move[key] = max(move[key], float(np.max(np.abs(np.asarray(a) - np.asarray(b)))))
        landings += np.bincount(hist["diag"]["landings"], minlength=4)
        first_kinds += np.bincount(np.array(hist["diag"]["first_is_entry"], int), minlength=2)
        print("%-22s V %5d nnz %5d distinct %4d calls %5d n_iter %3d winner %d" % (name, V, len(cols), len(hist["values"]), len(on), g.n_iter_, hist["winner"]))
    assert landings.min() > 0 and first_kinds.min() > 0, (landings, first_kinds)      # every place a trial draw can land, both kinds of first centre
    out.update(names=np.array(names), V=np.array(Vs, np.int64), umi_threshold=np.array(thrs, np.int64), row_ptr=np.array(ptr, np.int64),
               cols=np.concatenate(cols_all).astype(np.int64), vals=np.concatenate(vals_all).astype(np.int64), call_ptr=np.array(call_ptr, np.int64),
               calls=np.concatenate(calls_all).astype(np.int64), fitted=np.array(par["fitted"]), weights=np.array(par["w"], np.float64),
               means=np.array(par["mu"], np.float64), covariance=np.array(par["cov"], np.float64), n_iter=np.array(par["n_iter"], np.int64),
               lower_bound=np.array(par["lb"], np.float64), fixture_seed=np.array(par["seed"], np.int64), landings=landings, first_kinds=first_kinds,
               movement=np.array([max(move["ref_w"], move["form_w"]), max(move["ref_mu"], move["form_mu"]), max(move["ref_cov"], move["form_cov"])]),
               movement_reference=np.array([move["ref_w"], move["ref_mu"], move["ref_cov"]]),
               movement_forms=np.array([move["form_w"], move["form_mu"], move["form_cov"]]))
    # ---- the contaminant rule ----
    cc, order, flags, sources = contaminant_fixture(fa)
    rf, rsrc = R.identify_contaminants(cc, order)
    assert np.array_equal(rf, flags) and all(list(sources[t][sources[t] >= 0]) == rsrc[t] for t in range(len(flags))), (flags, rf, sources, rsrc)
    assert set(flags) == {0, 1, 2} and (sources >= 0).any()
    tot = cc.sum(1)
    assert flags[3] == 1 and tot[3] >= 1000 and tot[3] * 50 < tot.max() and flags[8] == 1 and tot[8] < 1000 and flags[9] == 2 and flags[11] == 0
    out.update(cont_counts=cc, cont_order=order, cont_flags=flags, cont_sources=sources)
    np.savez_compressed(OUT, **out)
    print("movement (weights, means, covariance): reference vs cell order", out["movement_reference"], "cell vs histogram order", out["movement_forms"])
    print("landings", landings, "first centre zero / entry", first_kinds, "->", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
