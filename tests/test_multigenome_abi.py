"""CPU-side checks of the multi-genome entry points (no GPU): the symbols are declared, exported and bound, they refuse a NULL
context, crgpu_multigenome_result has one layout in the header, the library (crgpu_abi_layout), the ctypes table, the Rust
block of INTEGRATION.md and include/crgpu.hpp, and crgpu_multigenome_summary (host f64) equals numpy on every number: the
per-sample inferred multiplets, np.mean (pairwise sum), the half-to-even rounding, the rates and both percentile bounds.

The struct is declared by tag, as crgpu_ordmag_result is (tests/test_cell_calling_abi.py says why)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import multigenome_numpy as R
import test_abi_and_host as A

ROOT = A.ROOT
NEW_SYMBOLS = ["crgpu_matrix_dev_genome_totals", "crgpu_multigenome_dev", "crgpu_multigenome_summary"]
EINVAL = -1
F1 = ([900, 800, 700, 650, 12, 3, 40, 0, 5], [10, 7, 0, 30, 600, 500, 40, 0, 450])
F2 = ([1200, 900, 2000, 1500, 0, 1100, 700, 1, 1300, 800, 950, 0], [0, 1, 2, 0, 1, 0, 0, 2, 1, 0, 0, 2])
F3 = ([500, 400, 450, 3], [2, 1, 350, 300])


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
    res, m = _lib.MultigenomeResult(), _lib.MatrixDevView()
    bc, tot = np.zeros(3, np.int64), np.zeros(2, np.uint64)
    assert L.crgpu_matrix_dev_genome_totals(None, C.byref(m), None, 0, 2, _lib.ptr(tot)) == EINVAL
    assert L.crgpu_multigenome_dev(None, None, None, 0, 1000, None, _lib.ptr(bc), None, None, C.byref(res)) == EINVAL
    # the summary needs no context; it refuses missing arrays and a sample count outside 1 .. the cap
    assert L.crgpu_multigenome_summary(None, 1, 5, None, C.byref(res)) == EINVAL
    assert L.crgpu_multigenome_summary(_lib.ptr(bc), 1, 5, None, None) == EINVAL
    assert L.crgpu_multigenome_summary(_lib.ptr(bc), 0, 5, None, C.byref(res)) == EINVAL
    assert L.crgpu_multigenome_summary(_lib.ptr(bc), _lib.MG_MAX_BOOTSTRAPS + 1, 5, None, C.byref(res)) == EINVAL
    assert _lib.MG_MAX_BOOTSTRAPS >= 1000


# ---- crgpu_multigenome_result: header == library == ctypes == Rust == C++ ------------------------------------------------------
def _header_struct():
    with open(os.path.join(ROOT, "include", "crgpu.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    m = re.search(r"\bstruct\s+crgpu_multigenome_result\s*\{(.*?)\}\s*;", text, flags=re.S)
    assert m and re.search(r"typedef\s+struct\s+crgpu_multigenome_result\s+crgpu_multigenome_result\s*;", text)
    fields = []
    for decl in m.group(1).split(";"):
        decl = " ".join(decl.split())
        if not decl:
            continue
        ctype, names = decl.split(" ", 1)
        for nm in names.split(","):
            size = A._C_SIZES[ctype]
            fields.append((nm.strip(), size, size, 1))
    return A._layout(fields)


def _rust_struct():
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        text = f.read()
    m = re.search(r"//\s*mirrors crgpu_multigenome_result[^\n]*\n#\[repr\(C\)\]\s*pub struct CrgpuMultigenomeResult\s*\{(.*?)\n\}", text, flags=re.S)
    assert m, "INTEGRATION.md has no CrgpuMultigenomeResult block"
    body = re.sub(r"//[^\n]*", "", m.group(1))
    fields = []
    for nm, ty in re.findall(r"pub\s+(\w+)\s*:\s*([^,]+?)\s*(?:,|$)", body.replace("\n", " ")):
        fields.append((nm, A._RUST_SIZES[ty.strip()], A._RUST_SIZES[ty.strip()], 1))
    return A._layout(fields)


def test_multigenome_result_layout_agrees_everywhere():
    from cellranger_amd import _lib

    size, align, fields = _header_struct()
    assert [f[0] for f in fields] == [
        "n", "obs_thresh0", "obs_thresh1", "observed_multiplets", "observed_genome0", "observed_genome1", "sum_c0_genome0",
        "sum_all_genome0", "sum_c1_genome1", "sum_all_genome1", "sum_max_single", "sum_all_single", "purity0", "purity1",
        "purity_overall", "boot_mean", "inferred_multiplets", "multiplet_rate", "normalized_multiplet_rate", "multiplet_rate_lb",
        "multiplet_rate_ub", "generator_words", "obs_branch", "rate_bounds_set"]
    assert (size, align) == (184, 8)
    lsize, lalign, lfields = A.library_layout("crgpu_multigenome_result")
    assert (size, align) == (lsize, lalign)
    assert [(o, s) for _, o, s in fields] == lfields
    cls = _lib.MultigenomeResult
    assert C.sizeof(cls) == size
    assert [(f[0], getattr(cls, f[0]).offset, getattr(cls, f[0]).size) for f in cls._fields_] == fields
    assert _rust_struct() == (size, align, fields)
    # include/crgpu.hpp uses the C struct itself and checks its size at compile time
    with open(os.path.join(ROOT, "include", "crgpu.hpp")) as f:
        hpp = f.read()
    assert re.search(r"static_assert\(sizeof\(crgpu_multigenome_result\) == %d\b" % size, hpp)
    assert not re.search(r"struct\s+\w*\s*\{[^}]*observed_multiplets", hpp)
    # the header's constants and the bindings'
    with open(os.path.join(ROOT, "include", "crgpu.h")) as f:
        hdr = f.read()
    assert int(re.search(r"#define CRGPU_MULTIGENOME_MAX_BOOTSTRAPS (\d+)", hdr).group(1)) == _lib.MG_MAX_BOOTSTRAPS
    for name, v in (("DEFAULT", 0), ("PERCENTILES", 1), ("DEFAULT_SUM", 2), ("PERCENTILES_SUM", 3)):
        assert int(re.search(r"#define CRGPU_MG_BRANCH_%s (\d)" % name, hdr).group(1)) == v == getattr(_lib, "MG_BRANCH_" + name)


# ---- crgpu_multigenome_summary == numpy ------------------------------------------------------------------------------------------
def _bits(x):
    return np.asarray(x, np.float64).view(np.uint64)


def _check_summary(bc, n):
    from cellranger_amd import engine as E

    ref = R.summary(bc, n)
    boot, got = E.multigenome_summary(bc, n)
    assert np.array_equal(_bits(boot), _bits(ref["boot"]))
    assert _bits(got["mean"]) == _bits(ref["mean"]) == _bits(np.mean(ref["boot"]))
    assert got["inferred_multiplets"] == ref["inferred_multiplets"]
    assert _bits(got["rate"]) == _bits(ref["rate"]) and _bits(got["normalized_rate"]) == _bits(ref["normalized_rate"])
    if len(bc) == 1:
        assert got["rate_lb"] is None and got["rate_ub"] is None and ref["rate_lb"] is None     # the flag is unset
    else:
        assert _bits(got["rate_lb"]) == _bits(ref["rate_lb"]) and _bits(got["rate_ub"]) == _bits(ref["rate_ub"])
    return got


@pytest.mark.parametrize("fixture", [F1, F2, F3], ids=["F1", "F2", "F3"])
def test_summary_of_the_fixtures_bootstrap_equals_numpy(fixture):
    counts, _, _ = R.bootstrap(*fixture)
    assert counts.shape == (1000, 3)
    got = _check_summary(counts, len(fixture[0]))
    if fixture is F2:      # five samples end at the cap min(mle, total)
        capped = [s for s, (m, g0, g1) in enumerate(counts.tolist())
                  if g0 and g1 and m / (2 * (g0 / (g0 + g1)) * (g1 / (g0 + g1))) > m + g0 + g1]
        assert len(capped) == 5 and got["inferred_multiplets"] == 1


@pytest.mark.parametrize("B", [1, 7, 8, 129, 1000, 2049])
def test_summary_of_random_triples_equals_numpy(B):
    rng = np.random.RandomState(B)
    n = 5000
    m = rng.randint(0, 400, B)
    g0 = rng.randint(0, 3000, B)
    g0[rng.rand(B) < 0.05] = 0
    bc = np.stack([m, g0, n - m - g0], axis=1).astype(np.int64)
    assert (bc >= 0).all()
    _check_summary(bc, n)
    _check_summary(bc, 0)          # a zero denominator: NaN rates on both sides
    small = np.stack([rng.randint(0, 9, B), rng.randint(0, 3, B), rng.randint(0, 3, B)], axis=1).astype(np.int64)   # caps and zero classes
    _check_summary(small, 13)


def test_rounding_is_half_to_even():
    from cellranger_amd import engine as E

    # (1, 5, 5) -> 2.0; (2, 2, 2) -> min(4, 6) = 4 ... means ending in .5
    for bc, mean, rounded in (([[1, 5, 5], [2, 3, 3]], 3.0, 3), ([[1, 5, 5], [0, 5, 5], [0, 5, 5], [0, 5, 5]], 0.5, 0),
                              ([[1, 5, 5], [1, 5, 5], [1, 5, 5], [0, 5, 5]], 1.5, 2), ([[1, 5, 5], [2, 2, 2], [1, 5, 5], [1, 5, 5]], 2.5, 2)):
        boot, got = E.multigenome_summary(np.array(bc), 10)
        ref = R.summary(np.array(bc), 10)
        assert got["mean"] == ref["mean"] == mean and got["inferred_multiplets"] == ref["inferred_multiplets"] == rounded
