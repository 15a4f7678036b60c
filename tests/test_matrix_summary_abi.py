"""CPU-side checks of the matrix-summary entry points (no GPU): the symbols are declared, exported and bound, they refuse a NULL
context and bad arguments, the two structs have one layout in the header, the library (crgpu_abi_layout), the ctypes table, the Rust
block of INTEGRATION.md and include/crgpu.hpp, and the host function crgpu_matrix_summary_stats equals the restatement
tests/matrix_summary_numpy.py on the hand cases and on 200 seeded random integer sets.  f64 values are compared as bit patterns, NaN
equal to NaN; the standard deviation is held within 4 ulp of the exact value (tests/test_matrix_summary_restatement.py says why), and
cv = std / mean within 5 * 2^-52 relative: 4 ulp of the std are at most 4 * 2^-52, the two divisions round by 2^-53 each."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import matrix_summary_numpy as R
import test_abi_and_host as A
import test_rtl_tags_abi as T
from test_matrix_summary_restatement import ulp_distance

ROOT = A.ROOT
NEW_SYMBOLS = ["crgpu_matrix_summary_dev", "crgpu_matrix_dev_reads_per_column", "crgpu_matrix_summary_stats"]
EINVAL, ERANGE = -1, -6
STRUCTS = {"crgpu_matrix_summary_class": ("MatrixSummaryClass", "CrgpuMatrixSummaryClass", 296),
           "crgpu_matrix_summary_floats": ("MatrixSummaryFloats", "CrgpuMatrixSummaryFloats", 120)}
EXACT = ("counts_mean", "counts_median", "counts_iqr", "genes_mean", "genes_median", "genes_iqr", "density", "cum_frac", "dupe_frac",
         "reads_per_cell", "reads_cum_frac")


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


def test_new_entry_points_refuse_a_null_context_and_bad_arguments():
    from cellranger_amd import _lib

    L = _lib.load()
    m, cls, out = _lib.MatrixDevView(), _lib.MatrixSummaryClass(), _lib.MatrixSummaryFloats()
    a64 = np.zeros(4, np.uint64)
    assert L.crgpu_matrix_summary_dev(None, C.byref(m), 4, 1, None, None, 0, None, None, _lib.ptr(a64), _lib.ptr(a64), C.byref(cls), None, None, None,
                                      None) == EINVAL
    assert L.crgpu_matrix_dev_reads_per_column(None, C.byref(m), 1, None) == EINVAL
    assert L.crgpu_matrix_summary_stats(None, 0, 0, C.byref(out)) == EINVAL
    assert L.crgpu_matrix_summary_stats(C.byref(cls), 0, 0, None) == EINVAL
    cls.n_cells = 1 << 32
    assert L.crgpu_matrix_summary_stats(C.byref(cls), 0, 0, C.byref(out)) == ERANGE
    assert b"2^32" in L.crgpu_last_error(None)
    assert (_lib.MS_MAX_CLASSES, _lib.MS_NO_CLASS, _lib.MS_TOP_N) == (32, 255, 5)


@pytest.mark.parametrize("name", sorted(STRUCTS))
def test_struct_layout_agrees_everywhere(name):
    from cellranger_amd import _lib

    cls_name, rust_name, expect = STRUCTS[name]
    size, align, fields = T._header_struct(name)
    assert (size, align) == (expect, 8)
    lsize, lalign, lfields = A.library_layout(name)
    assert (size, align) == (lsize, lalign)
    assert [(o, s) for _, o, s in fields] == lfields
    cls = getattr(_lib, cls_name)
    assert C.sizeof(cls) == size
    assert [(f[0], getattr(cls, f[0]).offset, getattr(cls, f[0]).size) for f in cls._fields_] == fields
    assert T._rust_struct(name, rust_name) == (size, align, fields)
    with open(os.path.join(ROOT, "include", "crgpu.hpp")) as f:
        hpp = f.read()
    assert re.search(r"static_assert\(sizeof\(%s\) == %d\b" % (name, size), hpp)      # crgpu.hpp uses the C struct itself
    with open(os.path.join(ROOT, "include", "crgpu.h")) as f:
        hdr = f.read()
    for macro, v in (("MAX_CLASSES", 32), ("NO_CLASS", 255), ("TOP_N", 5)):
        assert int(re.search(r"#define CRGPU_MS_%s (\d+)" % macro, hdr).group(1)) == v == getattr(_lib, "MS_" + macro)
    assert R.NO_CLASS == _lib.MS_NO_CLASS and R.TOP_N == _lib.MS_TOP_N


# ---- crgpu_matrix_summary_stats == restatement -------------------------------------------------------------------------------------
def _same_floats(got, ref):
    """every float of crgpu_matrix_summary_stats against R.class_floats"""
    for k in EXACT:
        a, b = got[k], ref[k]
        assert (math.isnan(a) and math.isnan(b)) or np.float64(a).view(np.uint64) == np.float64(b).view(np.uint64), (k, a, b)
    for pre in ("counts", "genes"):
        s, e = got[pre + "_std"], ref[pre + "_std"]
        assert (math.isnan(s) and math.isnan(e)) or ulp_distance(s, e) <= 4, (pre, s, e)
        cv, cv_ref = got[pre + "_cv"], ref[pre + "_cv"]
        assert (math.isnan(cv) and math.isnan(cv_ref)) or abs(cv - cv_ref) <= 5 * 2.0 ** -52 * cv_ref, (pre, cv, cv_ref)
        n = ref[pre + "_std_numpy"]      # np.std itself, where cv >= 1e-3: close, not equal
        if not math.isnan(n) and n >= 1e-3 * ref[pre + "_mean"]:
            assert abs(s - n) <= 64 * 2.0 ** -53 * n, (pre, s, n)


def test_stats_of_the_hand_cases():
    from cellranger_amd import engine as E

    fx = R.hand_matrix()
    for kw in ({}, {"cell_class_mask": np.array([1, 1, 0], np.uint32)}, {"reads": None}):
        s = R.run(fx, **kw)
        for c in s["classes"]:
            _same_floats(E.matrix_summary_stats(c, c["reads_cells"], s["reads_all"]), R.class_floats(c, c["reads_cells"], s["reads_all"]))
    c1 = R.run(fx)["classes"][1]
    got = E.matrix_summary_stats(c1, 90, 164)
    assert (got["counts_mean"], got["counts_median"], got["counts_iqr"], got["counts_std"], got["counts_cv"]) == (5.5, 5.5, 1.5, 1.5, 1.5 / 5.5)
    assert (got["density"], got["cum_frac"], got["dupe_frac"], got["reads_per_cell"], got["reads_cum_frac"]) == (1.0, 11 / 19, 1 - 11 / 90, 45.0, 90 / 164)


@pytest.mark.parametrize("block", range(4))
def test_stats_equal_the_restatement_on_random_integer_sets(block):
    from cellranger_amd import engine as E

    for seed in range(block * 50, block * 50 + 50):      # 200 in all
        rng = np.random.RandomState(seed)
        n = int(rng.choice([0, 1, 2, 3, 4, 5, 8, 101, rng.randint(6, 3000)]))
        hi = [3, 70000, 2 ** 32][seed % 3]
        x, g = rng.randint(0, hi, n).astype(np.int64), rng.randint(0, min(hi, 40000), n).astype(np.int64)
        xs, xq = R.moments(x)
        gs, gq = R.moments(g)
        nf = int(rng.randint(0, 40000))
        total = int(x.sum())
        c = dict(n_features_class=nf, n_cells=n, raw_total_counts=total + int(rng.randint(0, 3)) * int(rng.randint(0, 10 ** 6)),
                 cells_total_counts=total, cells_nnz=int(g.sum()), counts_sum=xs, counts_sumsq_hi=xq >> 64, counts_sumsq_lo=xq & (2 ** 64 - 1),
                 genes_sum=gs, genes_sumsq_hi=gq >> 64, genes_sumsq_lo=gq & (2 ** 64 - 1), counts_q=R.order_stats(x), genes_q=R.order_stats(g),
                 counts_per_cell=x, genes_per_cell=g)
        reads_cells = total + int(rng.randint(0, 2)) * int(rng.randint(0, 10 ** 7))
        reads_all = int(rng.randint(0, 2)) * (reads_cells + int(rng.randint(0, 10 ** 7)))
        _same_floats(E.matrix_summary_stats(c, reads_cells, reads_all), R.class_floats(c, reads_cells, reads_all))
