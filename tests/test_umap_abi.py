"""CPU-side checks of the UMAP entry points (no GPU): the symbols are declared, exported, bound and written into INTEGRATION.md; the two
structs have one layout in the header, the library (crgpu_abi_layout), the ctypes table, the Rust blocks of INTEGRATION.md and
include/crgpu.hpp; the ABI version is still 3; every refusal the header lists comes back as CRGPU_EINVAL without a context (with a
live context the refusal is the argument's and the device stays usable: tests/test_gpu_umap.py); the seams are fields, so umap.hip
holds no getenv and the README still says the library "reads these 32" environment variables; crgpu_umap_ab, which needs no device,
gives umap-learn's curve."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import test_abi_and_host as A
import test_subsample_abi as SA

ROOT = A.ROOT
NEW_SYMBOLS = ["crgpu_umap_ab", "crgpu_umap_graph_dev", "crgpu_umap_epochs_dev"]
EINVAL = -1
STRUCTS = {"crgpu_umap_args": ("UmapArgs", "CrgpuUmapArgs", 72), "crgpu_umap_result": ("UmapResult", "CrgpuUmapResult", 136)}


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
    assert int(re.search(r"#define CRGPU_UMAP_SLOTS (\d+)", hdr).group(1)) == 16 == _lib.UMAP_SLOTS
    assert int(re.search(r"#define CRGPU_UMAP_MAX_RATE (\d+)", hdr).group(1)) == 8 == _lib.UMAP_MAX_RATE
    section = hdr[hdr.index("---- RUN_UMAP"):hdr.index("#define CRGPU_UMAP_SLOTS")]
    for cited in ("stages/umap.rs", "sc_rna_analyzer.mro", "umap-learn", "no bit parity", "QUIRKS kept", "ONE SUM ORDER", "NOT covered: spectral"):
        assert cited in section, cited
    for left_out in ("spectral", "random stream", "set_op_mix_ratio", "local_connectivity", "H5 and CSV", "float32", "128 columns", "approximate"):
        assert left_out in section[section.index("NOT covered"):], left_out
    with open(os.path.join(ROOT, "README.md")) as f:
        readme = f.read()
    assert "reads these 32" in readme and "crgpu_umap_epochs_dev" in readme
    with open(os.path.join(ROOT, "cellranger_amd", "csrc", "umap.hip")) as f:
        src = f.read()
    assert "getenv" not in src and "atomicAdd" not in src and "hipGraph" not in src      # the seams are fields; no atomic, no capture
    for name in ("run_umap", "umap_ab", "umap_metric_input", "get_umap_name", "get_umap_key"):
        assert hasattr(engine, name), name
    for name in ("umap_graph", "umap_epochs"):
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


def test_the_curve_fit_needs_no_device():
    """crgpu_umap_ab at the stage's (0.3, 1): umap-learn's a = 0.99218, b = 1.11225 (scipy's defaults; the tight comparison is in
    tests/test_umap_restatement.py), no neighbouring (a, b) fits the 300 points better, and the refusals."""
    from cellranger_amd import _lib, engine

    L = _lib.load()
    a, b = C.c_double(), C.c_double()
    assert L.crgpu_umap_ab(0.3, 1.0, C.byref(a), C.byref(b)) == 0
    assert abs(a.value - 0.99218) < 1e-5 and abs(b.value - 1.11225) < 1e-5 and (a.value, b.value) == engine.umap_ab()
    x = np.linspace(0, 3, 300)

    def cost(p, q):
        return float(((1.0 / (1.0 + p * x ** (2 * q)) - np.where(x < 0.3, 1.0, np.exp(-(x - 0.3)))) ** 2).sum())

    for fa, fb in ((1.001, 1.0), (0.999, 1.0), (1.0, 1.001), (1.0, 0.999), (1.001, 1.001), (0.999, 1.001)):      # a least-squares fit: no neighbour does better
        assert cost(a.value, b.value) < cost(a.value * fa, b.value * fb), (fa, fb)
    for md, sp in ((-0.1, 1.0), (0.3, 0.0), (0.3, -1.0), (float("nan"), 1.0), (0.3, float("inf"))):
        assert L.crgpu_umap_ab(md, sp, C.byref(a), C.byref(b)) == EINVAL, (md, sp)
    assert L.crgpu_umap_ab(0.3, 1.0, None, C.byref(b)) == EINVAL and L.crgpu_umap_ab(0.3, 1.0, C.byref(a), None) == EINVAL


def _csr(n=8):
    """a ring: row i holds i - 1 and i + 1"""
    cols = np.sort(np.stack([(np.arange(n) - 1) % n, (np.arange(n) + 1) % n], axis=1), axis=1)
    return np.arange(n + 1, dtype=np.int64) * 2, cols.reshape(-1).astype(np.int32), np.full(2 * n, 0.5)


def test_entry_points_refuse_what_the_header_says():
    """Every refusal with a NULL context: CRGPU_EINVAL comes first for the missing context, so each call below is also made in order
    (8 rows, k = 3) and must give the same code -- what tells the refusals apart is the live context of tests/test_gpu_umap.py."""
    from cellranger_amd import _lib

    L = _lib.load()
    ptr = _lib.ptr
    ind = ((np.arange(8)[:, None] + np.arange(1, 4)[None]) % 8).astype(np.int32)
    dist = np.ones((8, 3)) * np.arange(1, 4)
    res = _lib.UmapResult()

    def graph(n=8, k=3, n_epochs=200, ind=ind, dist=dist):
        return L.crgpu_umap_graph_dev(None, ptr(ind), ptr(dist), n, k, n_epochs, C.byref(res))

    assert graph() == EINVAL      # NULL context, everything else in order
    bad_ind, twice, bad_dist = ind.copy(), ind.copy(), dist.copy()
    bad_ind[2, 1], twice[4, 2], bad_dist[3, 0] = 8, twice[4, 0], np.inf
    for kw in (dict(n=1), dict(n=1 << 31), dict(k=0), dict(k=8), dict(n=4000, k=1025), dict(n_epochs=0), dict(ind=bad_ind), dict(ind=twice),
               dict(dist=bad_dist), dict(dist=-dist)):
        assert graph(**kw) == EINVAL, kw
    assert L.crgpu_umap_graph_dev(None, None, ptr(dist), 8, 3, 200, C.byref(res)) == EINVAL
    assert L.crgpu_umap_graph_dev(None, ptr(ind), None, 8, 3, 200, C.byref(res)) == EINVAL
    assert L.crgpu_umap_graph_dev(None, ptr(ind), ptr(dist), 8, 3, 200, None) == EINVAL

    indptr, indices, values = _csr()
    y = np.random.RandomState(0).normal(size=(8, 2))

    def args(**kw):
        return _lib.UmapArgs(**dict(dict(a=1.0, b=1.0, n_run=2, n_epochs=10), **kw))

    def epochs(n=8, dims=2, indptr=indptr, indices=indices, values=values, y=y, a=None, state=None):
        a = a or args()
        s0, s1 = (np.ones(len(values)), np.ones(len(values))) if state is None else state
        return L.crgpu_umap_epochs_dev(None, ptr(indptr), ptr(indices), ptr(values), n, dims, ptr(y.copy()), ptr(s0.copy()), ptr(s1.copy()), C.byref(a),
                                       C.byref(res))

    assert epochs() == EINVAL
    out_of_range, descending, bad_ptr, nan_y, nan_v, zero_v = indices.copy(), indices.copy(), indptr.copy(), y.copy(), values.copy(), values.copy()
    out_of_range[5], bad_ptr[0], nan_y[4, 1], nan_v[3], zero_v[2] = 8, 1, np.nan, np.nan, 0.0
    descending[[2, 3]] = descending[[3, 2]]
    nan_state = (np.full(len(values), np.nan), np.ones(len(values)))
    for kw in (dict(n=1), dict(dims=1), dict(dims=4), dict(indices=out_of_range), dict(indices=descending), dict(indptr=bad_ptr), dict(y=nan_y),
               dict(values=nan_v), dict(values=zero_v), dict(a=args(a=0.0)), dict(a=args(b=-1.0)), dict(a=args(a=float("nan"))),
               dict(a=args(gamma=-1.0)), dict(a=args(initial_alpha=-1.0)), dict(a=args(negative_sample_rate=9)), dict(a=args(first_epoch=5, n_run=6)),
               dict(a=args(n_epochs=0, n_run=0)), dict(a=args(rows_per_wg=48)), dict(a=args(rows_per_wg=512)), dict(a=args(reserved0=1)),
               dict(a=args(reserved1=1)), dict(a=args(first_epoch=1), state=nan_state)):
        assert epochs(**kw) == EINVAL, kw
    a = args()
    s = np.ones(len(values))
    assert L.crgpu_umap_epochs_dev(None, None, ptr(indices), ptr(values), 8, 2, ptr(y.copy()), ptr(s), ptr(s), C.byref(a), C.byref(res)) == EINVAL
    assert L.crgpu_umap_epochs_dev(None, ptr(indptr), ptr(indices), ptr(values), 8, 2, ptr(y.copy()), None, ptr(s), C.byref(a), C.byref(res)) == EINVAL
    assert L.crgpu_umap_epochs_dev(None, ptr(indptr), ptr(indices), ptr(values), 8, 2, ptr(y.copy()), ptr(s), ptr(s), None, C.byref(res)) == EINVAL


def test_python_layer_refuses_before_the_library():
    from cellranger_amd import engine
    import umap_numpy as R

    out = engine.run_umap(None, R.TWO_ROWS.x)      # N = 2: zeros, and no context at all
    assert out["embedding"].shape == (2, 2) and not out["embedding"].any() and out["key"] == "2" and out["name"] == "gene_expression_2-d"
    assert out["n_epochs"] == 500 and out["nnz"] == 0 and (out["a"], out["b"]) == engine.umap_ab()
    one = engine.run_umap(None, np.zeros((1, 4)), umap_dims=3)
    assert one["embedding"].shape == (1, 3) and not one["embedding"].any()
    with pytest.raises(ValueError):
        engine.run_umap(None, np.zeros((300, 4)), umap_dims=4)
    with pytest.raises(ValueError, match="at most 128"):
        engine.run_umap(None, np.zeros((300, 129)))
    with pytest.raises(ValueError, match="metric"):
        engine.run_umap(None, np.zeros((300, 4)), metric="manhattan")
    with pytest.raises(ValueError, match="init"):
        engine.run_umap(None, np.zeros((300, 4)), init=np.zeros((300, 3)))
    with pytest.raises(ValueError, match="no start"):
        engine.run_umap(None, np.zeros((300, 1)))
