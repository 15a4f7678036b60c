"""CPU-side checks of the depth-normalisation entry points (no GPU): the symbols are declared, exported and bound, NULL arguments
are refused, crgpu_normalize_depth_args / crgpu_normalize_depth_result have one layout in the header, the library
(crgpu_abi_layout), the ctypes table, the Rust blocks of INTEGRATION.md and include/crgpu.hpp, and crgpu_normalize_depth_plan
equals the numpy restatement (tests/normalize_depth_numpy.py) exactly.  Patterned on tests/test_subsample_abi.py, whose parsers of
the header and of the Rust blocks it uses: both structs are declared by tag."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import normalize_depth_numpy as N
import test_abi_and_host as A
import test_subsample_abi as SA

ROOT = A.ROOT
NEW_SYMBOLS = ["crgpu_normalize_depth_dev", "crgpu_select_features_dev", "crgpu_normalize_depth_plan"]
EINVAL = -1


@pytest.fixture(scope="module", autouse=True)
def built_library():
    from cellranger_amd import build

    build.build()


def test_new_symbols_are_declared_exported_and_bound():
    from cellranger_amd import _lib

    declared = A.header_symbols()
    L = C.CDLL(_lib.LIB_PATH)
    for s in NEW_SYMBOLS:
        assert s in declared, s
        assert hasattr(L, s), s
        assert s in _lib.SYMBOLS, s
    assert _lib.load().crgpu_abi_version() == 3      # additive: no bump


def test_entry_points_refuse_null_arguments():
    from cellranger_amd import _lib

    L = _lib.load()
    a, res = _lib.NormalizeDepthArgs(), _lib.NormalizeDepthResult()
    assert L.crgpu_normalize_depth_dev(None, None, C.byref(a), C.byref(res)) == EINVAL
    mv = C.POINTER(_lib.MatrixDevView)()
    assert L.crgpu_select_features_dev(None, None, None, 0, C.byref(mv)) == EINVAL and not mv
    frac = np.zeros(2)
    assert L.crgpu_normalize_depth_plan(0, None, None, None, 1, 0, None, 1.0, _lib.ptr(frac)) == EINVAL
    assert L.crgpu_normalize_depth_plan(2, None, None, None, 1, 0, None, 1.0, _lib.ptr(frac)) == EINVAL
    t, x = np.zeros(2, np.uint32), np.ones(2)
    assert L.crgpu_normalize_depth_plan(2, _lib.ptr(t), _lib.ptr(x), _lib.ptr(x), 1, 0, None, 1.0, None) == EINVAL


@pytest.mark.parametrize("name,rust_name,cls_name,first,last,n_fields", [
    ("crgpu_normalize_depth_args", "CrgpuNormalizeDepthArgs", "NormalizeDepthArgs", "n_libs", "kept_out", 17),
    ("crgpu_normalize_depth_result", "CrgpuNormalizeDepthResult", "NormalizeDepthResult", "n_molecules", "tally_ms", 8)])
def test_struct_layout_agrees_everywhere(name, rust_name, cls_name, first, last, n_fields):
    from cellranger_amd import _lib

    size, align, fields = SA._header_struct(name)
    assert len(fields) == n_fields and fields[0][0] == first and fields[-1][0] == last
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


# ---- the plan: equal to the restatement ------------------------------------------------------------------------------------------------
HAND = [
    (dict(library_type=[0, 0, 1], usable_reads=[1000, 3000, 500], num_cells=[10, 10, 0]), [1.0, 100.0 / 300.0, 0.0]),
    (dict(library_type=[0, 1, 0], usable_reads=[1000, 3000, 500], num_cells=[10, 10, 0]), [0.0, 1.0, 0.0]),
    (dict(library_type=[0, 0], usable_reads=[1000, 4000], num_cells=[10, 10], targeted_aggr=True, is_targeted_lib=[0, 1],
          targeted_depth_factor=2.0), [1.0, 0.5]),
    (dict(library_type=[0, 0], usable_reads=[1000, 4000], num_cells=[10, 10], targeted_aggr=True, is_targeted_lib=[0, 1],
          targeted_depth_factor=5.0), [1.0, 0.25]),
    (dict(library_type=[0, 0, 1], usable_reads=[1000, 3000, 500], num_cells=[10, 10, 0], downsample=False), [1.0, 1.0, 1.0]),
]


def test_plan_on_the_hand_computed_cases():
    from cellranger_amd import engine as E

    for kw, want in HAND:
        got = E.normalize_depth_plan(**kw)
        assert np.array_equal(got, want), kw
        assert np.array_equal(got, N.plan(**kw)), kw


def test_plan_equals_the_restatement_on_random_inputs():
    from cellranger_amd import engine as E

    rng = np.random.default_rng(5)
    n_adjusted = n_refused = n_zero = 0
    for _ in range(200):
        n = int(rng.integers(1, 9))
        kw = dict(library_type=rng.integers(0, 3, n), usable_reads=rng.integers(0, 10 ** 9, n).astype(np.float64),
                  num_cells=rng.choice([0, 0, 1, 17, 5000, 12345], n).astype(np.float64), downsample=bool(rng.integers(0, 8)),
                  targeted_aggr=bool(rng.integers(0, 2)), is_targeted_lib=rng.integers(0, 2, n),
                  targeted_depth_factor=float(rng.choice([0.0, 0.5, 1.0, 1.7, 3.0])))
        if rng.integers(0, 4) == 0:
            kw["usable_reads"][rng.integers(0, n)] = 0.0
        want, got = N.plan(**kw), E.normalize_depth_plan(**kw)
        assert np.array_equal(got, want), kw
        plain = N.plan(**dict(kw, targeted_aggr=False))
        n_adjusted += not np.array_equal(want, plain)
        n_refused += kw["targeted_aggr"] and kw["downsample"] and np.array_equal(want, plain) and kw["targeted_depth_factor"] > 1 and want.any()
        n_zero += bool((want == 0).any())
    assert n_adjusted > 10 and n_refused > 5 and n_zero > 20             # the branches were reached


@pytest.mark.parametrize("bad", [dict(usable_reads=[1000.0, -1.0]), dict(usable_reads=[np.nan, 5.0]), dict(usable_reads=[np.inf, 5.0]),
                                 dict(num_cells=[-2.0, 10.0]), dict(num_cells=[np.nan, 10.0]),
                                 dict(targeted_aggr=True, targeted_depth_factor=np.nan), dict(targeted_aggr=True, targeted_depth_factor=-1.0),
                                 dict(targeted_aggr=True, targeted_depth_factor=np.inf)])
def test_plan_refuses_what_is_not_finite_or_negative(bad):
    from cellranger_amd import _lib
    from cellranger_amd import engine as E

    kw = dict(library_type=[0, 0], usable_reads=[1000.0, 4000.0], num_cells=[10.0, 10.0])
    kw.update(bad)
    with pytest.raises(_lib.CrgpuError) as e:
        E.normalize_depth_plan(**kw)
    assert e.value.code == EINVAL
