"""CPU-side checks of the t-SNE entry points (no GPU): the symbols are declared, exported, bound and written into INTEGRATION.md; the
two structs have one layout in the header, the library (crgpu_abi_layout), the ctypes table, the Rust blocks of INTEGRATION.md and
include/crgpu.hpp; the ABI version is still 3; CRGPU_TSNE_CAND_CHUNK is 4096 everywhere; every refusal the header lists comes back as
CRGPU_EINVAL without a context (with a live context the refusal is the argument's and the device stays usable:
tests/test_gpu_tsne.py); the seams are fields, so tsne.hip holds no getenv and the README still says the library "reads these 32"
environment variables."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import test_abi_and_host as A
import test_subsample_abi as SA

ROOT = A.ROOT
NEW_SYMBOLS = ["crgpu_tsne_affinities_dev", "crgpu_tsne_gradient_dev", "crgpu_tsne_dev"]
EINVAL = -1
STRUCTS = {"crgpu_tsne_args": ("TsneArgs", "CrgpuTsneArgs", 48), "crgpu_tsne_result": ("TsneResult", "CrgpuTsneResult", 168)}


@pytest.fixture(scope="module", autouse=True)
def built_library():
    from cellranger_amd import build

    build.build()


def test_new_symbols_are_declared_exported_and_bound():
    from cellranger_amd import _lib, engine

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
    assert int(re.search(r"#define CRGPU_TSNE_CAND_CHUNK (\d+)", hdr).group(1)) == 4096 == _lib.TSNE_CAND_CHUNK
    section = hdr[hdr.index("---- RUN_TSNE"):hdr.index("#define CRGPU_TSNE_CAND_CHUNK")]
    for cited in ("stages/analyzer/run_tsne/__init__.py", "bhtsne.py", "tsne.rs", "bh_tsne", "QUIRKS kept", "ONE SUM ORDER", "NOT covered: Barnes-Hut"):
        assert cited in section, cited
    for left_out in ("interpolation", "UMAP", "H5 and CSV", "random start", "float32", "128 columns"):
        assert left_out in section[section.index("NOT covered"):], left_out
    with open(os.path.join(ROOT, "README.md")) as f:
        readme = f.read()
    assert "reads these 32" in readme and "crgpu_tsne_dev" in readme
    with open(os.path.join(ROOT, "cellranger_amd", "csrc", "tsne.hip")) as f:
        src = f.read()
    assert "getenv" not in src and "atomicAdd" not in src and "hipGraph" not in src      # the seams are fields; no atomic, no capture
    for name in ("run_tsne", "tsne_feature_input", "get_tsne_name", "get_tsne_key"):
        assert hasattr(engine, name), name
    for name in ("tsne_affinities", "tsne_gradient", "tsne"):
        assert hasattr(engine.Context, name), name


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


def _csr(n=8):
    """a ring: row i holds i - 1 and i + 1"""
    cols = np.sort(np.stack([(np.arange(n) - 1) % n, (np.arange(n) + 1) % n], axis=1), axis=1)
    return np.arange(n + 1, dtype=np.int64) * 2, cols.reshape(-1).astype(np.int32), np.full(2 * n, 1.0 / (2 * n))


def test_entry_points_refuse_what_the_header_says():
    """Every refusal with a NULL context: CRGPU_EINVAL comes first for the missing context, so each call below is also made in order
    (8 rows, k = 3) and must give the same code -- what tells the refusals apart is the live context of tests/test_gpu_tsne.py."""
    from cellranger_amd import _lib

    L = _lib.load()
    ptr = _lib.ptr
    ind = ((np.arange(8)[:, None] + np.arange(1, 4)[None]) % 8).astype(np.int32)
    dist = np.ones((8, 3))
    res, a = _lib.TsneResult(), _lib.TsneArgs()

    def aff(n=8, k=3, perplexity=1.0, ind=ind, dist=dist, args=a):
        return L.crgpu_tsne_affinities_dev(None, ptr(ind), ptr(dist), n, k, perplexity, C.byref(args), C.byref(res))

    assert aff() == EINVAL      # NULL context, everything else in order
    bad_ind, bad_dist = ind.copy(), dist.copy()
    bad_ind[2, 1], bad_dist[3, 0] = 8, np.inf
    for kw in (dict(n=1), dict(n=1 << 31), dict(k=0), dict(k=8), dict(n=4000, k=1025), dict(perplexity=0.5), dict(perplexity=float("nan")),
               dict(ind=bad_ind), dict(dist=bad_dist), dict(dist=-dist), dict(args=_lib.TsneArgs(reserved=1))):
        assert aff(**kw) == EINVAL, kw
    assert L.crgpu_tsne_affinities_dev(None, None, ptr(dist), 8, 3, 1.0, C.byref(a), C.byref(res)) == EINVAL
    assert L.crgpu_tsne_affinities_dev(None, ptr(ind), None, 8, 3, 1.0, C.byref(a), C.byref(res)) == EINVAL
    assert L.crgpu_tsne_affinities_dev(None, ptr(ind), ptr(dist), 8, 3, 1.0, None, C.byref(res)) == EINVAL
    assert L.crgpu_tsne_affinities_dev(None, ptr(ind), ptr(dist), 8, 3, 1.0, C.byref(a), None) == EINVAL

    indptr, indices, values = _csr()
    y = np.random.RandomState(0).normal(size=(8, 2))

    def grad(n=8, dims=2, indptr=indptr, indices=indices, values=values, y=y, args=a, e=1.0):
        return L.crgpu_tsne_gradient_dev(None, ptr(indptr), ptr(indices), ptr(values), ptr(y), n, dims, e, C.byref(args), C.byref(res))

    def loop(n=8, dims=2, indptr=indptr, indices=indices, values=values, y=y, args=None):
        args = args or _lib.TsneArgs(first_iter=0, n_iters=2, max_iter=2)
        yy, uY, gains = y.copy(), np.zeros_like(y), np.ones_like(y)
        return L.crgpu_tsne_dev(None, ptr(indptr), ptr(indices), ptr(values), n, dims, ptr(yy), ptr(uY), ptr(gains), C.byref(args), C.byref(res))

    assert grad() == EINVAL and loop() == EINVAL
    out_of_range, descending, bad_ptr, nan_y, nan_v = indices.copy(), indices.copy(), indptr.copy(), y.copy(), values.copy()
    out_of_range[5], bad_ptr[0], nan_y[4, 1], nan_v[3] = 8, 1, np.nan, np.nan
    descending[[2, 3]] = descending[[3, 2]]
    for call in (grad, loop):
        for kw in (dict(n=1), dict(dims=1), dict(dims=4), dict(indices=out_of_range), dict(indices=descending), dict(indptr=bad_ptr), dict(y=nan_y),
                   dict(values=nan_v), dict(args=_lib.TsneArgs(row_tile=48, max_iter=9)), dict(args=_lib.TsneArgs(cand_tile=1025, max_iter=9)),
                   dict(args=_lib.TsneArgs(row_tile=64, slab_rows=96, max_iter=9)), dict(args=_lib.TsneArgs(reserved=1, max_iter=9))):
            assert call(**kw) == EINVAL, (call.__name__, kw)
    assert loop(args=_lib.TsneArgs(first_iter=5, n_iters=6, max_iter=10)) == EINVAL      # iterations beyond max_iter
    assert loop(args=_lib.TsneArgs(eta=-1.0, n_iters=1, max_iter=1)) == EINVAL
    assert grad(e=float("inf")) == EINVAL
    assert L.crgpu_tsne_gradient_dev(None, None, ptr(indices), ptr(values), ptr(y), 8, 2, 1.0, C.byref(a), C.byref(res)) == EINVAL
    assert L.crgpu_tsne_dev(None, ptr(indptr), ptr(indices), ptr(values), 8, 2, ptr(y.copy()), None, ptr(np.ones_like(y)), C.byref(a), C.byref(res)) == EINVAL


def test_python_layer_refuses_before_the_library():
    from cellranger_amd import engine

    class Matrix:      # MatrixDev.download() of 3 cells x 200 features
        def download(self):
            return None, np.array([0, 1, 2, 3]), np.array([0, 150, 199], np.int32), np.array([1, 2, 3], np.int32)

    with pytest.raises(ValueError, match="at most 128"):
        engine.tsne_feature_input(Matrix())

    class Small:
        def download(self):
            return None, np.array([0, 2, 2, 3]), np.array([0, 4, 1], np.int32), np.array([1, 3, 7], np.int32)

    x = engine.tsne_feature_input(Small(), n_features=5)
    assert x.shape == (3, 5) and x[0, 0] == 1.0 and x[0, 4] == 2.0 and x[2, 1] == 3.0 and x.sum() == 6.0
    # the all-zero case needs no context at all
    out = engine.run_tsne(None, np.random.RandomState(1).normal(size=(3, 4)))
    assert out["embedding"].shape == (3, 2) and not out["embedding"].any() and out["perplexity_used"] == 1 and out["key"] == "2"
    with pytest.raises(ValueError):
        engine.run_tsne(None, np.zeros((300, 4)), tsne_dims=4)
    with pytest.raises(ValueError, match="at most 128"):
        engine.run_tsne(None, np.zeros((300, 129)))
