"""CPU-side checks of the k-means entry points (no GPU): the symbols are declared, exported, bound and written into INTEGRATION.md; the
two structs have one layout in the header, the library (crgpu_abi_layout), the ctypes table, the Rust blocks of INTEGRATION.md and
include/crgpu.hpp; the ABI version is still 3; crgpu_kmeans_dev refuses a NULL context and, before it touches a device, K = 0, K > 64,
d > 128, n < K, a repeated K and ld < d (with a live context: tests/test_gpu_kmeans.py); crgpu_kmeans_db_index equals the restatement,
the 1e-3 clamp and a zero count included; the README names both environment switches."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import kmeans_numpy as R
import test_abi_and_host as A
import test_subsample_abi as SA

ROOT = A.ROOT
NEW_SYMBOLS = ["crgpu_kmeans_dev", "crgpu_kmeans_db_index", "crgpu_kmeans_seed_draws"]
EINVAL = -1
STRUCTS = {"crgpu_kmeans_args": ("KmeansArgs", "CrgpuKmeansArgs", 24), "crgpu_kmeans_result": ("KmeansResult", "CrgpuKmeansResult", 80)}


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
    for macro, v in (("MAX_K", 64), ("MAX_D", 128), ("MAX_LIST", 64)):
        assert int(re.search(r"#define CRGPU_KM_%s (\d+)" % macro, hdr).group(1)) == v == getattr(_lib, "KM_" + macro)
    assert "kmeans.py:67-95" in hdr and "1.7.2" in hdr and "NOT covered: the num_bcs subsample" in hdr
    with open(os.path.join(ROOT, "README.md")) as f:
        readme = f.read()
    assert "CRGPU_KM_BATCH" in readme and "CRGPU_KM_LDS_CENTERS" in readme and "reads these 32" in readme


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
    x = np.zeros((4, 3))
    a = _lib.KmeansArgs(init=None, tol_factor=1e-4, seed=0, max_iter=300)
    res = (_lib.KmeansResult * 2)()

    def call(ctx, n, d, ld, ks):
        ks = np.asarray(ks, np.uint32)
        return L.crgpu_kmeans_dev(ctx, _lib.ptr(x), n, d, ld, _lib.ptr(ks), len(ks), C.byref(a), res)

    assert call(None, 4, 3, 3, [2]) == EINVAL      # NULL context
    # K = 0, K > 64, d > 128, n < K, a repeated K, ld < d: the same code without a context (the message needs one: test_gpu_kmeans.py)
    for n, d, ld, ks in ((4, 3, 3, [0]), (4, 3, 3, [65]), (4, 129, 129, [2]), (4, 3, 3, [5]), (4, 3, 3, [2, 2]), (4, 3, 2, [2])):
        assert call(None, n, d, ld, ks) == EINVAL
    u, first = np.zeros(400), C.c_uint64(0)
    for seed, n, k in ((0, 0, 2), (0, 10, 0), (0, 10, 65)):
        assert L.crgpu_kmeans_seed_draws(seed, n, k, _lib.ptr(u), C.byref(first)) == EINVAL
    assert L.crgpu_kmeans_seed_draws(0, 10, 2, None, C.byref(first)) == EINVAL
    score = C.c_double(0.0)
    c, w, cnt = np.zeros((2, 2)), np.zeros(2), np.zeros(2, np.uint64)
    for k, d in ((0, 2), (65, 2), (2, 0), (2, 129)):
        assert L.crgpu_kmeans_db_index(k, d, _lib.ptr(c), _lib.ptr(w), _lib.ptr(cnt), C.byref(score)) == EINVAL
    assert L.crgpu_kmeans_db_index(2, 2, None, _lib.ptr(w), _lib.ptr(cnt), C.byref(score)) == EINVAL


def test_db_index_equals_the_restatement():
    from cellranger_amd import engine as E

    assert E.kmeans_db_index([[0.0, 0.0], [3.0, 4.0]], [8.0, 18.0], [2, 2]) == 1.0
    assert E.kmeans_db_index([[0.0], [1e-4]], [4.0, 4.0], [4, 0]) == 3.0 / 1e-3 == R.db_index(np.array([[0.0], [1e-4]]), [4.0, 4.0], [4, 0])
    rs = np.random.RandomState(17)
    for k, d in ((1, 1), (2, 10), (7, 3), (8, 5), (10, 10), (64, 128)):
        centers = rs.normal(size=(k, d))
        if k > 2:
            centers[k - 1] = centers[0] + 1e-6      # under the clamp
        wss = rs.uniform(1.0, 50.0, k)
        counts = rs.randint(0, 40, k).astype(np.uint64)
        counts[0] = 0
        assert E.kmeans_db_index(centers, wss, counts) == R.db_index(centers, wss, counts), (k, d)
