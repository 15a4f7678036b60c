"""The numpy restatement of RUN_PCA (tests/pca_numpy.py) against tests/golden/pca_reference.npz, on the CPU: the feature order, the
retry taken, the components used, `it` and `mprod` equal the reference's; the continuous outputs lie within 16 times the movement of the
reference itself between three orders of the cells (the bound of tests/test_gpu_pca.py), after the signs of the components are aligned
(the cosine with the reference's component must exceed 0.99 first); a permutation of the cells moves the restatement no further."""
import os

import numpy as np
import pytest

import pca_numpy as P

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pca_reference.npz"))
FACTOR = 16.0
_cache = {}


def _result(name):
    if name not in _cache:
        _cache[name] = P.run_stage(P.FIXTURES[name]["make"](), **P.fixture_args(name, int(GOLD[name + "_n_thresholded_bcs"])))
    return _cache[name]


def _rel(got, ref):
    fin = np.isfinite(ref)
    assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(got[~fin & ~np.isnan(ref)], ref[~fin & ~np.isnan(ref)])
    return float(np.abs(got[fin] - ref[fin]).max() / np.abs(ref[fin]).max()) if fin.any() else 0.0


@pytest.mark.parametrize("name", sorted(P.FIXTURES))
def test_discrete_outputs(name):
    r, retried = _result(name)
    assert retried == bool(GOLD[name + "_retried"]) and r["n_components"] == int(GOLD[name + "_n_components"])
    assert np.array_equal(r["features_selected"], GOLD[name + "_features_selected"])
    assert (r["it"], r["mprod"]) == (int(GOLD[name + "_it"]), int(GOLD[name + "_mprod"]))
    assert r["n_thresholded_bcs"] == int(GOLD[name + "_n_thresholded_bcs"])


@pytest.mark.parametrize("name", sorted(P.FIXTURES))
def test_continuous_outputs(name):
    r, _ = _result(name)
    signs, cos = P.align_signs(r["components"], GOLD[name + "_components"])
    assert cos.min() > 0.99
    got = dict(d=r["d"], variance_explained=r["variance_explained"], components=r["components"] * signs[:, None],
               transformed=r["transformed_pca_matrix"] * signs[None, :], dispersion=r["dispersion"])
    for key, g in got.items():
        dev, bound = _rel(g, GOLD["%s_%s" % (name, key)]), FACTOR * float(GOLD["%s_mov_%s" % (name, key)])
        print("%-12s %-20s deviation %.3g bound %.3g" % (name, key, dev, bound))
        assert dev <= bound, (name, key, dev, bound)


@pytest.mark.parametrize("name", ["w257", "constructed"])
def test_a_permutation_of_the_cells_moves_nothing_discrete(name):
    r, _ = _result(name)
    dense = P.FIXTURES[name]["make"]()
    order = np.random.RandomState(7).permutation(dense.shape[1])
    q, _ = P.run_stage(dense, cell_order=order, **P.fixture_args(name))
    assert (q["it"], q["mprod"]) == (r["it"], r["mprod"]) and np.array_equal(q["features_selected"], r["features_selected"])
    signs, cos = P.align_signs(q["components"], r["components"])
    assert cos.min() > 0.99
    assert _rel(q["transformed_pca_matrix"] * signs[None, :], r["transformed_pca_matrix"]) <= FACTOR * float(GOLD[name + "_mov_transformed"])
