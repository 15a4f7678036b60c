"""CPU-side checks of the marginal-calls entry points (no GPU): the symbols are declared, exported, bound and written into
INTEGRATION.md; the two structs have one layout in the header, the library (crgpu_abi_layout), the ctypes table, the Rust blocks of
INTEGRATION.md and include/crgpu.hpp; the device entry points refuse a NULL context and umi_threshold 0; the seed hook equals numpy's
RandomState(0); crgpu_tag_contaminants equals the restatement on the golden fixture and on a NaN-correlation case; the README names
the new environment switch.  All equalities are of integers or of doubles that numpy and the library produce by the same operations
(the 53-bit doubles of MT19937, sequential sums of 1 / V), so they are asserted bit for bit."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import marginal_calls_numpy as R
import test_abi_and_host as A
import test_subsample_abi as SA
from test_marginal_calls_restatement import golden

ROOT = A.ROOT
NEW_SYMBOLS = ["crgpu_marginal_calls_dev", "crgpu_marginal_calls_free", "crgpu_tag_moments_dev", "crgpu_tag_contaminants", "crgpu_marginal_seed_draws"]
EINVAL, ERANGE = -1, -6
STRUCTS = {"crgpu_marginal_row": ("MarginalRow", "CrgpuMarginalRow", 96), "crgpu_marginal_calls": ("MarginalCalls", "CrgpuMarginalCalls", 152)}


@pytest.fixture(scope="module", autouse=True)
def built_library():
    from cellranger_amd import build

    build.build()


def test_new_symbols_are_declared_exported_and_bound():
    from cellranger_amd import _lib

    declared = A.header_symbols()
    L = C.CDLL(_lib.LIB_PATH)
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        text = f.read()
    for s in NEW_SYMBOLS:
        assert s in declared and hasattr(L, s) and s in _lib.SYMBOLS, s
        assert re.search(r"pub fn %s\(" % s, text), s
    assert _lib.load().crgpu_abi_version() == 3      # additive: no bump
    with open(os.path.join(ROOT, "include", "crgpu.h")) as f:
        hdr = f.read()
    for macro, v in (("INITS", 10), ("SKIPPED", 0), ("FITTED", 1)):
        assert int(re.search(r"#define CRGPU_MC_%s (\d+)" % macro, hdr).group(1)) == v == getattr(_lib, "MC_" + macro)
    assert "feature_assigner.py:213-230" in hdr and "1.7.2" in hdr
    assert not re.search(r"CALL_TAGS_MARGINAL \(its\s+\*?\s*calls are an input\)", hdr)      # no longer an input
    with open(os.path.join(ROOT, "README.md")) as f:
        assert "CRGPU_MC_LDS_VALUES" in f.read()


def test_entry_points_refuse_null_and_threshold_zero():
    from cellranger_amd import _lib

    L = _lib.load()
    rows = np.zeros(1, np.uint32)
    out = C.POINTER(_lib.MarginalCalls)()
    mv = _lib.MatrixDevView()
    assert L.crgpu_marginal_calls_dev(None, C.byref(mv), _lib.ptr(rows), 1, 4, 1, 0, C.byref(out)) == EINVAL
    # umi_threshold 0 would assign zeros: CRGPU_EINVAL as well (with a live context: tests/test_gpu_marginal_calls.py)
    assert L.crgpu_marginal_calls_dev(None, C.byref(mv), _lib.ptr(rows), 1, 4, 0, 0, C.byref(out)) == EINVAL and not out
    x = np.zeros(1, np.uint64)
    assert L.crgpu_tag_moments_dev(None, C.byref(mv), _lib.ptr(rows), 1, 4, _lib.ptr(x), _lib.ptr(x), _lib.ptr(x)) == EINVAL
    L.crgpu_marginal_calls_free(None, None)      # a no-op
    u, f = np.zeros(30), np.zeros(10, np.uint64)
    assert L.crgpu_marginal_seed_draws(0, _lib.ptr(u), _lib.ptr(f)) == EINVAL and L.crgpu_marginal_seed_draws(5, None, _lib.ptr(f)) == EINVAL
    fl, src, o = np.zeros(2, np.uint8), np.zeros(4, np.int32), np.array([0, 0], np.uint32)
    s1, s2 = np.ones(2, np.uint64), np.ones(4, np.uint64)
    assert L.crgpu_tag_contaminants(2, 5, _lib.ptr(s1), _lib.ptr(s1), _lib.ptr(s2), _lib.ptr(o), 1000, 50.0, 0.5, _lib.ptr(fl), _lib.ptr(src)) == EINVAL      # not a permutation
    assert L.crgpu_tag_contaminants(17, 5, _lib.ptr(s1), _lib.ptr(s1), _lib.ptr(s2), _lib.ptr(o), 1000, 50.0, 0.5, _lib.ptr(fl), _lib.ptr(src)) == ERANGE


@pytest.mark.parametrize("name", sorted(STRUCTS))
def test_struct_layout_agrees_everywhere(name):
    from cellranger_amd import _lib

    cls_name, rust_name, expect = STRUCTS[name]
    size, align, fields = SA._header_struct(name)
    assert (size, align) == (expect, 8)
    lsize, lalign, lfields = A.library_layout(name)
    assert (size, align) == (lsize, lalign)
    assert [(o, s) for _, o, s in fields] == lfields
    cls = getattr(_lib, cls_name)
    assert C.sizeof(cls) == size
    assert [(f[0], getattr(cls, f[0]).offset, getattr(cls, f[0]).size) for f in cls._fields_] == fields
    assert SA._rust_struct(name, rust_name) == (size, align, fields)
    with open(os.path.join(ROOT, "include", "crgpu.hpp")) as f:
        hpp = f.read()
    assert re.search(r"static_assert\(sizeof\(%s\) == %d\b" % (name, size), hpp)


@pytest.mark.parametrize("V", [2, 3, 1000, 2 ** 17 + 1])
def test_seed_draws_equal_numpy(V):
    from cellranger_amd import engine as E

    u, first = E.marginal_seed_draws(V)
    rs = np.random.RandomState(0)
    want_u, want_first = np.zeros((10, 3)), np.zeros(10, np.int64)
    for j in range(10):      # numpy's own choice() and uniform(), the calls scikit-learn makes
        state = rs.get_state()
        want_first[j] = rs.choice(V, p=np.full(V, 1.0) / np.full(V, 1.0).sum())
        probe = np.random.RandomState()
        probe.set_state(state)
        want_u[j, 0] = probe.random_sample()
        want_u[j, 1:] = rs.uniform(size=2)
    assert u.tobytes() == want_u.tobytes() and np.array_equal(first.astype(np.int64), want_first)
    ru, rf = R.seed_draws(V)
    assert u.tobytes() == ru.tobytes() and np.array_equal(first.astype(np.int64), rf)
    assert u.ravel()[:30].tobytes() == golden()["draws"].tobytes()


def _moments(c):
    c = np.asarray(c, np.int64)
    return c.sum(1), (c * c).sum(1), c @ c.T


def test_contaminants_equal_the_restatement():
    from cellranger_amd import engine as E

    g = golden()
    c, order = g["cont_counts"], g["cont_order"]
    flags, src = E.tag_contaminants(*_moments(c), c.shape[1], order)
    rf, rs = R.identify_contaminants(c, order)
    assert np.array_equal(flags, rf) and src == rs and np.array_equal(flags, g["cont_flags"])
    assert set(flags.tolist()) == {0, 1, 2} and any(src)
    # a NaN correlation (a constant tag) is skipped; the tag that follows another gets it as its source
    c = np.array([[900, 0, 900, 0], [5, 5, 5, 5], [450, 0, 450, 1]], np.int64) * 3
    flags, src = E.tag_contaminants(*_moments(c), 4, [0, 1, 2], min_counts=10)
    assert (list(flags), src) == ([0, 1, 1], [[], [], [0]]) == (list(R.identify_contaminants(c, [0, 1, 2], min_counts=10)[0]), R.identify_contaminants(c, [0, 1, 2], min_counts=10)[1])
    # the order of the visit decides which of two equal tags loses: the later one in sorted-id order
    c = np.array([[100, 0, 100, 0], [100, 0, 100, 0]], np.int64) * 10
    for order, loser in (([0, 1], 1), ([1, 0], 0)):
        flags, src = E.tag_contaminants(*_moments(c), 4, order)
        rf, rs = R.identify_contaminants(c, order)
        assert list(flags) == list(rf) and src == rs and flags[loser] == 1 and flags[1 - loser] == 0
