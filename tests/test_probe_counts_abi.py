"""CPU: the probe x barcode entry points (BcUmiInfo::probe_counts, cr_types/src/types.rs:190-204, and what is built on it)
are declared in include/crgpu.h, exported from libcrgpu.so, bound by the ctypes table, and refuse a NULL context."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("crgpu_counts_probe_triplets_dev", "crgpu_counts_probe_triplets", "crgpu_assemble_probe_matrix_dev",
                "crgpu_probe_metrics_dev")
EINVAL = -1


def setup_module(module):
    from cellranger_amd import build

    build.build()


def test_probe_entry_points_are_declared_and_exported():
    from cellranger_amd import _lib

    with open(os.path.join(ROOT, "include", "crgpu.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    L = C.CDLL(_lib.LIB_PATH)
    for name in ENTRY_POINTS:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name + " is not declared in include/crgpu.h"
        assert hasattr(L, name), name + " is not exported"
        assert name in _lib.SYMBOLS, name + " is not in the ctypes table"
    for stat in ("CRGPU_STAT_PROBE_SEGMENTS_WAVE", "CRGPU_STAT_PROBE_SEGMENTS_WORKGROUP", "CRGPU_STAT_PROBE_SEGMENTS_GLOBAL"):
        assert re.search(r"#define\s+%s\s+\d+" % stat, text), stat


def test_probe_entry_points_refuse_a_null_context():
    from cellranger_amd import _lib

    L = _lib.load()
    n = C.c_uint64(7)
    a, b, c = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert L.crgpu_counts_probe_triplets_dev(None, None, 10, C.byref(a), C.byref(b), C.byref(c), C.byref(n)) == EINVAL
    assert L.crgpu_counts_probe_triplets(None, None, 10, None, None, None, C.byref(n)) == EINVAL
    out = C.POINTER(_lib.MatrixDevView)()
    assert L.crgpu_assemble_probe_matrix_dev(None, None, 10, None, 0, C.byref(out)) == EINVAL
    assert L.crgpu_probe_metrics_dev(None, None, 10, None, 0, None, None) == EINVAL
    assert n.value == 7 and not out


def test_cpp_mirror_declares_probe_counts():
    with open(os.path.join(ROOT, "include", "crgpu.hpp")) as f:
        text = f.read()
    assert re.search(r"struct\s+ProbeBarcodeCount\b", text)
    assert re.search(r"std::vector<ProbeBarcodeCount>\s+probe_counts\b", text)
