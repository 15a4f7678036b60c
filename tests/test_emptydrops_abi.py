"""CPU-side checks of the EmptyDrops entry points (no GPU): the symbols are declared, exported and bound, they refuse a NULL
context, crgpu_sgt_proportions (host code) equals the numpy restatement, and crgpu_emptydrops_result / crgpu_emptydrops_arrays
have one layout in the header, the library (crgpu_abi_layout), the ctypes table, the Rust blocks of INTEGRATION.md and
include/crgpu.hpp.  Patterned on tests/test_cell_calling_abi.py: both structs are declared by tag."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import emptydrops_numpy as R
import test_abi_and_host as A
from test_emptydrops_restatement import GOLDEN, RTOL

ROOT = A.ROOT
NEW_SYMBOLS = ["crgpu_sgt_proportions", "crgpu_emptydrops_dev", "crgpu_ambient_pvalues_dev", "crgpu_emptydrops_arrays_free",
               "crgpu_emptydrops_simulate_dev"]
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


def test_new_entry_points_refuse_a_null_context():
    from cellranger_amd import _lib

    L = _lib.load()
    res, arr, m, n = _lib.EmptydropsResult(), _lib.EmptydropsArrays(), _lib.MatrixDevView(), C.c_uint64()
    assert L.crgpu_emptydrops_dev(None, C.byref(m), None, 0, None, None, 0, 0, 10, 500, 100, 0.01, 0, None, 0, None, 0, C.byref(res),
                                  C.byref(arr)) == EINVAL
    assert L.crgpu_ambient_pvalues_dev(None, None, None, 0, None, 0, None, 0, 0.01, None, None, None, None, C.byref(n)) == EINVAL
    L.crgpu_emptydrops_arrays_free(None, C.byref(arr))          # a no-op, not a crash
    nd = C.c_uint32()
    assert L.crgpu_emptydrops_simulate_dev(None, None, 0, None, None, 0, 1, 0, None, C.byref(nd), None, None, None) == EINVAL


# ---- crgpu_sgt_proportions == the restatement -------------------------------------------------------------------------------------
def _zipf_counts(seed, n_items, total, power):
    rs = np.random.RandomState(seed)
    p = 1.0 / np.arange(1, n_items + 1) ** power
    return rs.multinomial(total, p / p.sum())


@pytest.mark.parametrize("case", ["fixture", "zero_class", "no_zero_class"])
def test_sgt_proportions_equal_the_restatement(case):
    """the same measured-then-fixed relative tolerance as the restatement against the reference (RTOL)"""
    from cellranger_amd import engine as E

    if case == "fixture":
        prof = np.load(GOLDEN)["profile"]
    elif case == "zero_class":
        prof = _zipf_counts(3, 2000, 100_000, 1.2)
    else:
        prof = _zipf_counts(4, 400, 100_000, 1.2)
    assert (prof == 0).any() == (case != "no_zero_class")
    freq = prof[prof > 0]
    pstar, p0, slope = R.sgt_proportions(freq)
    got, gp0, gslope, status = E.sgt_proportions(freq)
    assert status == 0
    assert np.all(np.abs(got - pstar) <= RTOL * pstar) and abs(gp0 - p0) <= RTOL * p0 and abs(gslope - slope) <= RTOL * abs(slope)
    assert abs(got.sum() + gp0 - 1.0) < 1e-12
    if case == "fixture":
        g = np.load(GOLDEN)
        assert np.all(np.abs(got - g["ref_pstar"]) <= RTOL * g["ref_pstar"]) and abs(gp0 - float(g["ref_p0"])) <= RTOL * gp0


def test_sgt_refusals_are_status_codes():
    from cellranger_amd import _lib
    from cellranger_amd import engine as E

    few = np.array([1, 1, 1, 2, 2, 3, 4, 5, 6, 7, 8, 9], np.uint64)          # 9 distinct frequencies
    with pytest.raises(R.SimpleGoodTuringError):
        R.sgt_proportions(few)
    got, _, _, status = E.sgt_proportions(few)
    assert got is None and status == _lib.SGT_TOO_FEW
    flat = np.repeat(np.arange(1, 41), 3).astype(np.uint64)                   # every frequency equally often: slope ~ 0
    with pytest.raises(R.SimpleGoodTuringError) as ei:
        R.sgt_proportions(flat)
    got, _, slope, status = E.sgt_proportions(flat)
    assert got is None and status == _lib.SGT_SLOPE and slope > -1 and abs(slope - ei.value.slope) <= 1e-12
    for bad in (np.zeros(0, np.uint64), np.array([3, 0, 2], np.uint64)):
        with pytest.raises(E.CrgpuError) as e2:
            E.sgt_proportions(bad)
        assert e2.value.code == EINVAL


# ---- the two structs: header == library == ctypes == Rust == C++ ------------------------------------------------------------------
def _header_struct(name):
    with open(os.path.join(ROOT, "include", "crgpu.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    m = re.search(r"\bstruct\s+%s\s*\{(.*?)\}\s*;" % name, text, flags=re.S)
    assert m and re.search(r"typedef\s+struct\s+%s\s+%s\s*;" % (name, name), text)
    fields = []
    for decl in m.group(1).split(";"):
        decl = " ".join(decl.split())
        if not decl:
            continue
        ctype, names = decl.split(" ", 1)
        for nm in names.split(","):
            nm = nm.strip()
            size = 8 if nm.startswith("*") else A._C_SIZES[ctype]
            fields.append((nm.lstrip("* "), size, size, 1))
    return A._layout(fields)


def _rust_struct(name, rust_name):
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        text = f.read()
    m = re.search(r"//\s*mirrors %s[^\n]*\n#\[repr\(C\)\]\s*pub struct %s\s*\{(.*?)\n\}" % (name, rust_name), text, flags=re.S)
    assert m, "INTEGRATION.md has no %s block" % rust_name
    body = re.sub(r"//[^\n]*", "", m.group(1))
    fields = []
    for nm, ty in re.findall(r"pub\s+(\w+)\s*:\s*([^,]+?)\s*(?:,|$)", body.replace("\n", " ")):
        ty = ty.strip()
        size = 8 if ty.startswith("*mut") or ty.startswith("*const") else A._RUST_SIZES[ty]
        fields.append((nm, size, size, 1))
    return A._layout(fields)


@pytest.mark.parametrize("name,rust_name,cls_name,first,last,n_fields", [
    ("crgpu_emptydrops_result", "CrgpuEmptydropsResult", "EmptydropsResult", "status", "sim_ms", 12),
    ("crgpu_emptydrops_arrays", "CrgpuEmptydropsArrays", "EmptydropsArrays", "n_candidates", "d_sim_loglk", 17)])
def test_struct_layout_agrees_everywhere(name, rust_name, cls_name, first, last, n_fields):
    from cellranger_amd import _lib

    size, align, fields = _header_struct(name)
    assert len(fields) == n_fields and fields[0][0] == first and fields[-1][0] == last
    if name == "crgpu_emptydrops_result":
        assert {"status", "n_ambient_used", "max_background_umis", "emptydrops_minimum_umis", "n_eval_features", "n_candidates",
                "n_distinct_n", "n_nonambient", "sgt_slope", "sgt_p0"} <= {f[0] for f in fields}
    lsize, lalign, lfields = A.library_layout(name)
    assert (size, align) == (lsize, lalign)
    assert [(o, s) for _, o, s in fields] == lfields
    cls = getattr(_lib, cls_name)
    assert C.sizeof(cls) == size
    assert [(f[0], getattr(cls, f[0]).offset, getattr(cls, f[0]).size) for f in cls._fields_] == fields
    assert _rust_struct(name, rust_name) == (size, align, fields)
    with open(os.path.join(ROOT, "include", "crgpu.hpp")) as f:
        hpp = f.read()
    assert re.search(r"static_assert\(sizeof\(%s\) == %d\b" % (name, size), hpp)
    assert not re.search(r"struct\s+\w*\s*\{[^}]*\b(n_ambient_used|d_pvalues_adj)\b\s*;", hpp)      # no second declaration


def test_status_codes_of_header_and_binding_agree():
    from cellranger_amd import _lib

    with open(os.path.join(ROOT, "include", "crgpu.h")) as f:
        text = f.read()
    d = dict(re.findall(r"#define\s+(CRGPU_(?:ED|SGT)_\w+)\s+(\d+)", text))
    assert [int(d[k]) for k in ("CRGPU_ED_OK", "CRGPU_ED_NO_AMBIENT", "CRGPU_ED_SGT_NOT_APPLICABLE", "CRGPU_ED_NO_CELLS",
                                "CRGPU_ED_NO_CANDIDATES")] == [0, 1, 2, 3, 4] == sorted(_lib.ED_STATUS)
    assert (int(d["CRGPU_SGT_TOO_FEW"]), int(d["CRGPU_SGT_SLOPE"])) == (_lib.SGT_TOO_FEW, _lib.SGT_SLOPE)
    assert (int(d["CRGPU_ED_KEEP_PROFILE"]), int(d["CRGPU_ED_KEEP_SIM_TABLE"])) == (_lib.ED_KEEP_PROFILE, _lib.ED_KEEP_SIM_TABLE)
