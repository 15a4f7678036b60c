"""CPU-side checks of the k-nearest-neighbour entry points (no GPU): the symbols are declared, exported, bound and written into
INTEGRATION.md; the two structs have one layout in the header, the library (crgpu_abi_layout), the ctypes table, the Rust blocks of
INTEGRATION.md and include/crgpu.hpp; the ABI version is still 3; CRGPU_KNN_MAX_K is 1024 everywhere; crgpu_knn_dev refuses a NULL
context and k = 0, k >= n, k > 1024, d = 0, d > 128, ld < d, n < 2 and a query range outside the rows (with a live context, where the
refusal is the argument's and the device stays usable: tests/test_gpu_knn.py); the seams are fields, so the README still says the
library "reads these 32" environment variables."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import test_abi_and_host as A
import test_subsample_abi as SA

ROOT = A.ROOT
NEW_SYMBOLS = ["crgpu_knn_dev", "crgpu_graphclust_num_neighbors"]
EINVAL = -1
STRUCTS = {"crgpu_knn_args": ("KnnArgs", "CrgpuKnnArgs", 32), "crgpu_knn_result": ("KnnResult", "CrgpuKnnResult", 96)}


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
    assert int(re.search(r"#define CRGPU_KNN_MAX_K (\d+)", hdr).group(1)) == 1024 == _lib.KNN_MAX_K
    for cited in ("stages/analyzer/run_graph_clustering/__init__.py", "graphclust.py:39-62", "graphclust.py:95-106", "1.7.2", "TIE RULE", "QUIRK kept",
                  "NOT covered: Louvain and `convert`"):
        assert cited in hdr, cited
    section = hdr[hdr.index("NOT covered: Louvain"):hdr.index("#define CRGPU_KNN_MAX_K")]
    for left_out in ("SNN", "num_bcs", "MERGE_CLUSTERS", "H5 and CSV", "float32", "PCA"):
        assert left_out in section, left_out
    with open(os.path.join(ROOT, "README.md")) as f:
        readme = f.read()
    assert "reads these 32" in readme and "crgpu_knn_dev" in readme
    with open(os.path.join(ROOT, "cellranger_amd", "csrc", "knn.hip")) as f:
        src = f.read()
    assert "getenv" not in src and "lower index" in src      # the seams are fields; the source states the quirk


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


def test_entry_points_refuse_what_the_header_says():
    from cellranger_amd import _lib

    L = _lib.load()
    x = np.zeros((8, 4))
    res = _lib.KnnResult()

    def call(n, d, ld, k, q0=0, nq=0):
        a = _lib.KnnArgs(query_start=q0, n_queries=nq)
        return L.crgpu_knn_dev(None, _lib.ptr(x), n, d, ld, k, C.byref(a), C.byref(res))

    assert call(8, 4, 4, 3) == EINVAL      # NULL context, everything else in order
    # k = 0, k >= n, k > 1024, d = 0, d > 128, ld < d, n < 2, a query range outside the rows: the same code without a context
    for args in ((8, 4, 4, 0), (8, 4, 4, 8), (4000, 4, 4, 1025), (8, 0, 4, 3), (8, 129, 129, 3), (8, 4, 3, 3), (1, 4, 4, 1), (8, 4, 4, 3, 8, 1),
                 (8, 4, 4, 3, 6, 3), (8, 4, 4, 3, 2, 0)):
        assert call(*args) == EINVAL, args
    a = _lib.KnnArgs()
    assert L.crgpu_knn_dev(None, None, 8, 4, 4, 3, C.byref(a), C.byref(res)) == EINVAL
    assert L.crgpu_knn_dev(None, _lib.ptr(x), 8, 4, 4, 3, None, C.byref(res)) == EINVAL
    assert L.crgpu_knn_dev(None, _lib.ptr(x), 8, 4, 4, 3, C.byref(a), None) == EINVAL
    k = C.c_uint32(7)
    for n in (0, 1):
        assert L.crgpu_graphclust_num_neighbors(n, 1, -230.0, 120.0, C.byref(k)) == EINVAL
    assert L.crgpu_graphclust_num_neighbors(100, 1, -230.0, 120.0, None) == EINVAL
    assert L.crgpu_graphclust_num_neighbors(100, 1, float("nan"), 120.0, C.byref(k)) == EINVAL
    assert L.crgpu_graphclust_num_neighbors(100, 1, -230.0, 120.0, C.byref(k)) == 0 and k.value == 10
