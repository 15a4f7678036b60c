"""CPU-side checks of the aggregate stage's entry points (no GPU): the symbols are declared, exported and bound; crgpu_aggregates_info
has one layout in the header, the library (crgpu_abi_layout), the ctypes table, the Rust block of INTEGRATION.md and include/crgpu.hpp;
the two host functions equal numpy bit for bit; NULL contexts and bad arguments are refused."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import aggregates_numpy as R
import test_abi_and_host as A
import test_rtl_tags_abi as T

NEW_SYMBOLS = ["crgpu_aggregate_min_antibodies", "crgpu_antigen_outlier_threshold", "crgpu_aggregates_by_counts_dev",
               "crgpu_aggregates_highly_corrected_dev", "crgpu_counts_corrected_reads_per_column", "crgpu_aggregates_antigen_outliers_dev",
               "crgpu_aggregates_partition_dev", "crgpu_take_columns_dev", "crgpu_sum_u32_dev", "crgpu_filter_cells_min_umis_dev",
               "crgpu_filter_cells_mito_dev"]
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
        assert s in declared and hasattr(L, s) and s in _lib.SYMBOLS, s
    assert _lib.load().crgpu_abi_version() == 3      # additive: no bump


def test_info_struct_layout_agrees_everywhere():
    from cellranger_amd import _lib

    name = "crgpu_aggregates_info"
    size, align, fields = T._header_struct(name)
    assert (size, align) == (48, 8)
    lsize, lalign, lfields = A.library_layout(name)
    assert (size, align) == (lsize, lalign) and [(o, s) for _, o, s in fields] == lfields
    cls = _lib.AggregatesInfo
    assert C.sizeof(cls) == size
    assert [(f[0], getattr(cls, f[0]).offset, getattr(cls, f[0]).size) for f in cls._fields_] == fields
    assert T._rust_struct(name, "CrgpuAggregatesInfo") == (size, align, fields)
    with open(os.path.join(A.ROOT, "include", "crgpu.hpp")) as f:
        assert re.search(r"static_assert\(sizeof\(%s\) == %d\b" % (name, size), f.read())
    with open(os.path.join(A.ROOT, "include", "crgpu.h")) as f:
        hdr = f.read()
    for macro, v in (("KIND_OTHER", 0), ("KIND_ANTIBODY", 1), ("KIND_ANTIGEN", 2), ("COUNTS", 1), ("HIGHLY_CORRECTED", 2), ("ANTIGEN", 4)):
        assert int(re.search(r"#define CRGPU_AGG_%s (\d+)" % macro, hdr).group(1)) == v == getattr(_lib, "AGG_" + macro) == getattr(R, macro)


def test_every_rust_declaration_is_there():
    with open(os.path.join(A.ROOT, "INTEGRATION.md")) as f:
        text = f.read()
    for s in NEW_SYMBOLS:
        assert re.search(r"pub fn %s\(" % s, text), s


def test_min_antibodies_against_numpy_for_0_to_64():
    from cellranger_amd import engine as E

    for n in range(65):
        frac = 0.6 if n > 26 else -0.02 * n + 1.1
        assert E.aggregate_min_antibodies(n) == int(np.round(n * frac)) == R.min_antibodies(n), n
    assert [E.aggregate_min_antibodies(n) for n in (5, 9, 13, 25, 26, 27, 30)] == [5, 8, 11, 15, 15, 16, 18]


def test_antigen_threshold_against_numpy_bit_for_bit():
    from cellranger_amd import engine as E

    rng = np.random.RandomState(5)
    cases = [rng.randint(0, hi, n) for hi in (3, 50, 5000, 2 ** 31) for n in (1, 2, 3, 4, 5, 7, 64, 99, 100)]
    cases += [np.full(n, v) for n in (1, 100) for v in (0, 7, 2 ** 32 - 1)]
    cases += [np.array([0] * 55 + [400] * 40 + [2500] * 5)]
    for x in cases:
        x = x.astype(np.uint32)
        q1, q3, thr = E.antigen_outlier_threshold(x)
        top = np.sort(x).astype(np.int64)
        e3, e1 = np.quantile(top, 0.75), np.quantile(top, 0.25)
        exp = (e1, e3, e3 + (e3 - e1) * 3)
        assert np.array([q1, q3, thr]).tobytes() == np.array(exp, np.float64).tobytes(), (x, (q1, q3, thr), exp)
        assert np.array(R.antigen_threshold(x), np.float64).tobytes() == np.array(exp, np.float64).tobytes()


def test_refusals_without_a_context():
    from cellranger_amd import _lib

    L = _lib.load()
    m, info, n32, n64, p, d = _lib.MatrixDevView(), _lib.AggregatesInfo(), C.c_uint32(), C.c_uint64(), C.c_void_p(), C.c_double()
    kind = np.zeros(4, np.uint8)
    assert L.crgpu_aggregate_min_antibodies(5, None) == EINVAL
    assert L.crgpu_antigen_outlier_threshold(None, 3, None, None, C.byref(d)) == EINVAL
    assert L.crgpu_antigen_outlier_threshold(_lib.ptr(np.zeros(3, np.uint32)), 0, None, None, C.byref(d)) == EINVAL
    assert L.crgpu_antigen_outlier_threshold(_lib.ptr(np.zeros(3, np.uint32)), 3, None, None, None) == EINVAL
    assert L.crgpu_aggregates_by_counts_dev(None, C.byref(m), _lib.ptr(kind), 4, 1, None, None, 0, C.byref(n32), C.byref(info)) == EINVAL
    assert L.crgpu_aggregates_highly_corrected_dev(None, None, None, 0, None, C.byref(n64)) == EINVAL
    assert L.crgpu_counts_corrected_reads_per_column(None, None, C.byref(m), 1, None) == EINVAL
    assert L.crgpu_aggregates_antigen_outliers_dev(None, C.byref(m), _lib.ptr(kind), 4, None, None, 0, C.byref(n32), C.byref(d)) == EINVAL
    assert L.crgpu_aggregates_partition_dev(None, None, 0, C.byref(p), C.byref(n64), C.byref(p), C.byref(n64)) == EINVAL
    assert L.crgpu_take_columns_dev(None, None, 4, 0, None, 0, None) == EINVAL
    assert L.crgpu_sum_u32_dev(None, None, 0, C.byref(n64)) == EINVAL
    assert L.crgpu_filter_cells_min_umis_dev(None, None, 0, None, 0, 0, C.byref(p), C.byref(n64)) == EINVAL
    assert L.crgpu_filter_cells_mito_dev(None, None, None, 0, None, 0, 5.0, C.byref(p), C.byref(n64), C.byref(p), C.byref(n64)) == EINVAL
