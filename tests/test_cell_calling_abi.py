"""CPU-side checks of the cell-calling entry points (no GPU): the symbols are declared, exported and bound, they refuse a NULL
context, the candidate grid of the estimate equals numpy's, and crgpu_ordmag_result has one layout in the header, the library
(crgpu_abi_layout), the ctypes table, the Rust block of INTEGRATION.md and include/crgpu.hpp.

tests/test_abi_and_host.py pins the exact set of `typedef struct { ... } name;` blocks of the header, so the new struct is
declared by tag (`struct crgpu_ordmag_result { ... };` + typedef) and its Rust mirror carries its marker comment above the
block; this file compares the four views of it with that test's own layout helpers."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import test_abi_and_host as A

ROOT = A.ROOT
NEW_SYMBOLS = ["crgpu_matrix_dev_column_sums", "crgpu_ordmag_candidates", "crgpu_call_cells_ordmag_dev", "crgpu_cell_ranks_dev",
               "crgpu_select_barcodes_cols_dev", "crgpu_mt19937_stream_dev"]
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
    res, cols, n, mv = _lib.OrdmagResult(), C.c_void_p(), C.c_uint64(), C.POINTER(_lib.MatrixDevView)()
    m = _lib.MatrixDevView()
    assert L.crgpu_matrix_dev_column_sums(None, C.byref(m), None, 0, None) == EINVAL
    assert L.crgpu_call_cells_ordmag_dev(None, None, 0, 0, 1 << 18, 0, C.byref(res), C.byref(cols), C.byref(n)) == EINVAL
    assert L.crgpu_cell_ranks_dev(None, C.byref(m), None, 0, None) == EINVAL
    assert L.crgpu_select_barcodes_cols_dev(None, C.byref(m), None, 0, C.byref(mv)) == EINVAL
    assert L.crgpu_mt19937_stream_dev(None, 0, 0, None, C.byref(n), None) == EINVAL


@pytest.mark.parametrize("max_expected_cells", [2, 50, 1000, 45_000, 80_000, 1 << 18])
def test_candidate_grid_equals_numpy(max_expected_cells):
    from cellranger_amd import _lib
    from cellranger_amd import engine as E

    expect = np.unique(np.round(np.power(2, np.linspace(1, np.log2(max_expected_cells), 2000))).astype(int))
    got = E.ordmag_candidates(max_expected_cells)
    assert got.dtype == np.int64 and np.array_equal(got, expect)
    if max_expected_cells == 1 << 18:
        assert len(got) == 1414 and list(got[:3]) == [2, 3, 4] and list(got[-2:]) == [260603, 262144]
    L, n = _lib.load(), C.c_uint32()
    assert L.crgpu_ordmag_candidates(max_expected_cells, None, 0, C.byref(n)) == 0 and n.value == len(expect)   # size query
    if len(expect) > 1:
        small = np.zeros(len(expect) - 1, np.int64)
        assert L.crgpu_ordmag_candidates(max_expected_cells, _lib.ptr(small), len(small), C.byref(n)) == -6      # CRGPU_ERANGE
    assert L.crgpu_ordmag_candidates(1, None, 0, C.byref(n)) == EINVAL
    assert L.crgpu_ordmag_candidates(max_expected_cells, None, 0, None) == EINVAL


# ---- crgpu_ordmag_result: header == library == ctypes == Rust == C++ ------------------------------------------------------------
def _header_struct():
    with open(os.path.join(ROOT, "include", "crgpu.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    m = re.search(r"\bstruct\s+crgpu_ordmag_result\s*\{(.*?)\}\s*;", text, flags=re.S)
    assert m and re.search(r"typedef\s+struct\s+crgpu_ordmag_result\s+crgpu_ordmag_result\s*;", text)
    fields = []
    for decl in m.group(1).split(";"):
        decl = " ".join(decl.split())
        if not decl:
            continue
        ctype, names = decl.split(" ", 1)
        for nm in names.split(","):
            nm = nm.strip()
            arr = re.match(r"(\w+)\[(\d+)\]$", nm)
            size = A._C_SIZES[ctype]
            fields.append((arr.group(1) if arr else nm, size, size, int(arr.group(2)) if arr else 1))
    return A._layout(fields)


def _rust_struct():
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        text = f.read()
    m = re.search(r"//\s*mirrors crgpu_ordmag_result[^\n]*\n#\[repr\(C\)\]\s*pub struct CrgpuOrdmagResult\s*\{(.*?)\n\}", text, flags=re.S)
    assert m, "INTEGRATION.md has no CrgpuOrdmagResult block"
    body = re.sub(r"//[^\n]*", "", m.group(1))
    fields = []
    for nm, ty in re.findall(r"pub\s+(\w+)\s*:\s*([^,]+?)\s*(?:,|$)", body.replace("\n", " ")):
        arr = re.match(r"\[(\w+);\s*(\d+)\]$", ty.strip())
        base = arr.group(1) if arr else ty.strip()
        fields.append((nm, A._RUST_SIZES[base], A._RUST_SIZES[base], int(arr.group(2)) if arr else 1))
    return A._layout(fields)


def test_ordmag_result_layout_agrees_everywhere():
    from cellranger_amd import _lib

    size, align, fields = _header_struct()
    assert [f[0] for f in fields] == ["n_nonzero", "recovered_cells", "recovered_boot", "loss_boot", "baseline_bc_idx", "top_n_boot",
                                      "filtered_bcs_mean", "filtered_bcs_var", "filtered_bcs_cv", "filtered_bcs_lb", "filtered_bcs_ub",
                                      "filtered_bcs", "filtered_bcs_cutoff", "filtered_bcs_cutoff_set", "estimated"]
    assert dict((f[0], f[2]) for f in fields)["top_n_boot"] == 800
    # the library
    lsize, lalign, lfields = A.library_layout("crgpu_ordmag_result")
    assert (size, align) == (lsize, lalign)
    assert [(o, s) for _, o, s in fields] == lfields
    # the ctypes table
    cls = _lib.OrdmagResult
    assert C.sizeof(cls) == size
    assert [(f[0], getattr(cls, f[0]).offset, getattr(cls, f[0]).size) for f in cls._fields_] == fields
    # the Rust mirror of INTEGRATION.md
    assert _rust_struct() == (size, align, fields)
    # include/crgpu.hpp uses the C struct itself (no second declaration that could drift) and checks its size at compile time
    with open(os.path.join(ROOT, "include", "crgpu.hpp")) as f:
        hpp = f.read()
    assert re.search(r"static_assert\(sizeof\(crgpu_ordmag_result\) == %d\b" % size, hpp)
    assert not re.search(r"struct\s+\w*[Oo]rdmag\w*\s*\{[^}]*recovered_boot", hpp)
