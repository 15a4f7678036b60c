"""CPU-side checks of the read-subsampling entry points (no GPU): the symbols are declared, exported and bound,
crgpu_subsample_dev refuses a NULL context, and crgpu_subsample_args / crgpu_subsample_result have one layout in the header,
the library (crgpu_abi_layout), the ctypes table, the Rust blocks of INTEGRATION.md and include/crgpu.hpp.  Patterned on
tests/test_emptydrops_abi.py: both structs are declared by tag."""
import ctypes as C
import os
import re

import pytest

import test_abi_and_host as A

ROOT = A.ROOT
NEW_SYMBOLS = ["crgpu_subsample_dev", "crgpu_subsample_plan", "crgpu_subsample_summary"]
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
    a, res, n = _lib.SubsampleArgs(), _lib.SubsampleResult(), C.c_uint32(7)
    assert L.crgpu_subsample_dev(None, None, C.byref(a), C.byref(res)) == EINVAL
    assert L.crgpu_subsample_plan(0, None, 0, 0, None, None, None, None, 0, 10, None, None, 0, C.byref(n)) == EINVAL and n.value == 0
    assert L.crgpu_subsample_summary(1, 1, 0, 0, None, None, None, None, None, None, None, None, None, None) == EINVAL


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
        decl = re.sub(r"^const\s+", "", decl)
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
    ("crgpu_subsample_args", "CrgpuSubsampleArgs", "SubsampleArgs", "n_tasks", "any_reads", 19),
    ("crgpu_subsample_result", "CrgpuSubsampleResult", "SubsampleResult", "n_molecules", "draw_ms", 8)])
def test_struct_layout_agrees_everywhere(name, rust_name, cls_name, first, last, n_fields):
    from cellranger_amd import _lib

    size, align, fields = _header_struct(name)
    assert len(fields) == n_fields and fields[0][0] == first and fields[-1][0] == last
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


def test_constants_of_header_and_binding_agree():
    from cellranger_amd import _lib

    with open(os.path.join(ROOT, "include", "crgpu.h")) as f:
        text = f.read().replace("\\\n", " ")
    d = dict(re.findall(r"#define\s+(CRGPU_SS_\w+)\s+(\d+)\b", text))
    assert [int(d[k]) for k in ("CRGPU_SS_PER_CELL", "CRGPU_SS_CELLS_ONLY", "CRGPU_SS_BULK")] == [_lib.SS_PER_CELL, _lib.SS_CELLS_ONLY, _lib.SS_BULK]
    assert [int(d[k]) for k in ("CRGPU_SS_PLAN_RAW", "CRGPU_SS_PLAN_MAPPED", "CRGPU_SS_PLAN_RAW_CELLS", "CRGPU_SS_PLAN_BULK")] == \
        [_lib.SS_PLAN_RAW, _lib.SS_PLAN_MAPPED, _lib.SS_PLAN_RAW_CELLS, _lib.SS_PLAN_BULK]
    assert int(d["CRGPU_SS_NUM_ADDITIONAL_DEPTHS"]) == _lib.SS_NUM_ADDITIONAL_DEPTHS and int(d["CRGPU_SS_SUMMARY_COLS"]) == len(_lib.SS_SUMMARY_COLS)
    lists = {k: tuple(int(x) for x in v.split(",")) for k, v in re.findall(r"#define\s+(CRGPU_SS_\w*FIXED_DEPTHS)\s+\{([^}]*)\}", text)}
    assert lists == {"CRGPU_SS_FIXED_DEPTHS": _lib.SS_FIXED_DEPTHS, "CRGPU_SS_TARGETED_FIXED_DEPTHS": _lib.SS_TARGETED_FIXED_DEPTHS,
                     "CRGPU_SS_BULK_FIXED_DEPTHS": _lib.SS_BULK_FIXED_DEPTHS}
