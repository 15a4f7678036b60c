"""CPU-side checks of the CORRECT_CHEMISTRY_BATCH entry points (no GPU): the symbols are declared, exported, bound and written into
INTEGRATION.md; the four structs have one layout in the header, the library (crgpu_abi_layout), the ctypes table, the Rust blocks of
INTEGRATION.md and include/crgpu.hpp; the ABI version is still 3; CRGPU_BC_PAIR_CHUNK is 2048 everywhere; the seams are fields (no
getenv in batch_correction.hip or knn.hip, the README still says the library "reads these 32" environment variables); crgpu_mnn_pairs
equals the set arithmetic of join() on random lists, empty intersections included; every refusal of crgpu_knn_cross_dev and
crgpu_batch_correct_dev comes back as CRGPU_EINVAL without a context (with a live one, where the refusal is the argument's and the
device stays usable: tests/test_gpu_batch_correction.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import test_abi_and_host as A
import test_subsample_abi as SA

ROOT = A.ROOT
NEW_SYMBOLS = ["crgpu_knn_cross_dev", "crgpu_mnn_pairs", "crgpu_batch_correct_dev"]
EINVAL = -1
STRUCTS = {"crgpu_knn_cross_args": ("KnnCrossArgs", "CrgpuKnnCrossArgs", 48), "crgpu_bc_step": ("BcStep", "CrgpuBcStep", 48),
           "crgpu_bc_args": ("BcArgs", "CrgpuBcArgs", 16), "crgpu_bc_result": ("BcResult", "CrgpuBcResult", 96)}


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
    assert int(re.search(r"#define CRGPU_BC_PAIR_CHUNK (\d+)", hdr).group(1)) == 2048 == _lib.BC_PAIR_CHUNK
    assert hdr.index("int crgpu_graphclust_num_neighbors(") < hdr.index("CORRECT_CHEMISTRY_BATCH") < hdr.index("int crgpu_knn_cross_dev(")
    section = hdr[hdr.index("CORRECT_CHEMISTRY_BATCH"):hdr.index("#define CRGPU_BC_PAIR_CHUNK")]
    for cited in ("correct_chemistry_batch/__init__.py", "analysis/batch_correction.py", "QUIRK kept", "gamma = 0.5 * sigma", "NOT covered"):
        assert cited in section, cited
    for left_out in ("batches smaller than knn", "H5, CSV and pickle", "float32", "PCA"):
        assert left_out in section[section.index("NOT covered"):], left_out
    with open(os.path.join(ROOT, "README.md")) as f:
        readme = f.read()
    assert "reads these 32" in readme and "crgpu_batch_correct_dev" in readme
    for name in ("batch_correction.hip", "knn.hip"):
        with open(os.path.join(ROOT, "cellranger_amd", "csrc", name)) as f:
            src = f.read()
        assert "getenv" not in src, name                               # the seams are fields


@pytest.mark.parametrize("name", sorted(STRUCTS))
def test_struct_layout_agrees_everywhere(name):
    from cellranger_amd import _lib

    cls_name, rust_name, expect = STRUCTS[name]
    size, align, fields = SA._header_struct(name)
    assert (size, align) == (expect, 8 if name != "crgpu_bc_args" else 4)
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


def _mnn(a, start_i, b, start_j, capacity=None):
    from cellranger_amd import _lib

    a, b = np.ascontiguousarray(a, np.int32), np.ascontiguousarray(b, np.int32)
    cap = a.size if capacity is None else capacity
    pairs = np.full((max(cap, 1), 2), -7, np.int32)
    m, n1, n2 = C.c_uint64(99), C.c_uint64(99), C.c_uint64(99)
    rc = _lib.load().crgpu_mnn_pairs(_lib.ptr(a), a.shape[0], start_i, _lib.ptr(b), b.shape[0], start_j, a.shape[1], _lib.ptr(pairs), cap,
                                     C.byref(m), C.byref(n1), C.byref(n2))
    return rc, pairs[:min(m.value, cap)], m.value, n1.value, n2.value


@pytest.mark.parametrize("seed,n_i,n_j,k,start_i,start_j", [(1, 40, 30, 3, 0, 40), (2, 7, 90, 5, 100, 3), (3, 25, 25, 1, 0, 25), (4, 12, 9, 9, 50, 20),
                                                            (5, 300, 200, 10, 0, 300)])
def test_mnn_pairs_equals_the_set_arithmetic(seed, n_i, n_j, k, start_i, start_j):
    rs = np.random.RandomState(seed)
    a = np.stack([rs.choice(n_j, k, replace=False) for _ in range(n_i)]) + start_j
    b = np.stack([rs.choice(n_i, k, replace=False) for _ in range(n_j)]) + start_i
    nn_ij = set(zip(np.repeat(np.arange(n_i) + start_i, k).tolist(), a.ravel().tolist()))
    nn_ji = {(y, x) for x, y in zip(np.repeat(np.arange(n_j) + start_j, k).tolist(), b.ravel().tolist())}
    want = sorted(nn_ij & nn_ji)
    rc, pairs, m, n1, n2 = _mnn(a, start_i, b, start_j)
    assert rc == 0 and m == len(want) and [tuple(p) for p in pairs.tolist()] == want
    assert n1 == len({p for p, _ in want}) and n2 == len({q for _, q in want})
    from cellranger_amd import engine as E

    got, e1, e2 = E.mnn_pairs(a, start_i, b, start_j)
    assert got.dtype == np.int32 and got.shape == (len(want), 2) and [tuple(p) for p in got.tolist()] == want and (e1, e2) == (n1, n2)


def test_mnn_pairs_edge_cases_and_refusals():
    from cellranger_amd import _lib

    # no mutual pair at all: the rows of i name row 12 but for row 1, which names 13; 12 names row 1, every other row of j names 0
    a = np.array([[12], [13], [12], [12], [12], [12]], np.int32)
    b = np.array([[0], [0], [1], [0]], np.int32)
    rc, pairs, m, n1, n2 = _mnn(a, 0, b, 10)
    assert (rc, m, n1, n2) == (0, 0, 0, 0) and len(pairs) == 0
    b[3] = 1                                                           # now 13 names row 1 back
    rc, pairs, m, n1, n2 = _mnn(a, 0, b, 10)
    assert (rc, m, n1, n2) == (0, 1, 1, 1) and pairs.tolist() == [[1, 13]]
    # a repeated entry is one pair: the reference's pairs are a set
    rc, pairs, m, n1, n2 = _mnn(np.array([[3, 3]]), 0, np.array([[0, 0]] * 4), 1)
    assert (rc, m, n1, n2) == (0, 1, 1, 1) and pairs.tolist() == [[0, 3]]
    # counted only; a capacity that is too small says how many there are
    L = _lib.load()
    m, n1, n2 = C.c_uint64(), C.c_uint64(), C.c_uint64()
    aa, bb = np.array([[2, 3], [2, 3]], np.int32), np.array([[0, 1], [0, 1]], np.int32)
    assert L.crgpu_mnn_pairs(_lib.ptr(aa), 2, 0, _lib.ptr(bb), 2, 2, 2, None, 0, C.byref(m), C.byref(n1), C.byref(n2)) == 0
    assert (m.value, n1.value, n2.value) == (4, 2, 2)
    rc, pairs, count, _, _ = _mnn(aa, 0, bb, 2, capacity=3)
    assert rc == EINVAL and count == 4 and pairs.tolist() == [[0, 2], [0, 3], [1, 2]]
    # an index outside its batch, k = 0, an empty batch, a NULL
    assert _mnn(np.array([[4]]), 0, np.array([[0]]), 1)[0] == EINVAL and _mnn(np.array([[0]]), 0, np.array([[0]]), 1)[0] == EINVAL
    assert _mnn(np.array([[1]]), 0, np.array([[1]]), 1)[0] == EINVAL and _mnn(np.array([[1]]), 0, np.array([[-1]]), 1)[0] == EINVAL
    one = np.array([[1]], np.int32)
    zero = np.array([[0]], np.int32)
    args = [_lib.ptr(one), 1, 0, _lib.ptr(zero), 1, 1, 1, None, 0, C.byref(m), C.byref(n1), C.byref(n2)]
    assert L.crgpu_mnn_pairs(*args) == 0
    for pos, bad in ((0, None), (3, None), (1, 0), (4, 0), (6, 0), (9, None), (10, None), (11, None), (2, 1 << 31)):
        call = list(args)
        call[pos] = bad
        assert L.crgpu_mnn_pairs(*call) == EINVAL, pos


def test_entry_points_refuse_what_the_header_says():
    from cellranger_amd import _lib

    L = _lib.load()
    x = np.zeros((8, 4))
    x[:, 0] = np.arange(8)
    res = _lib.KnnResult()

    def cross(n, d, ld, k, q0=0, nq=4, c0=4, nc=4, **seams):
        a = _lib.KnnCrossArgs(query_start=q0, n_queries=nq, cand_start=c0, n_cands=nc, **seams)
        return L.crgpu_knn_cross_dev(None, _lib.ptr(x), n, d, ld, k, C.byref(a), C.byref(res))

    assert cross(8, 4, 4, 3) == EINVAL      # NULL context, everything else in order
    # k = 0, k > n_cands, k > 1024, d = 0, d > 128, ld < d, n = 0, a range outside the rows, an empty range: the same code without a context
    for args in ((8, 4, 4, 0), (8, 4, 4, 5), (4000, 4, 4, 1025), (8, 0, 4, 3), (8, 129, 129, 3), (8, 4, 3, 3), (0, 4, 4, 3), (8, 4, 4, 3, 8, 1),
                 (8, 4, 4, 3, 6, 3), (8, 4, 4, 3, 0, 0), (8, 4, 4, 3, 0, 4, 8, 1), (8, 4, 4, 3, 0, 4, 6, 3), (8, 4, 4, 3, 0, 4, 4, 0)):
        assert cross(*args) == EINVAL, args
    a = _lib.KnnCrossArgs(n_queries=4, cand_start=4, n_cands=4)
    assert L.crgpu_knn_cross_dev(None, None, 8, 4, 4, 3, C.byref(a), C.byref(res)) == EINVAL
    assert L.crgpu_knn_cross_dev(None, _lib.ptr(x), 8, 4, 4, 3, None, C.byref(res)) == EINVAL
    assert L.crgpu_knn_cross_dev(None, _lib.ptr(x), 8, 4, 4, 3, C.byref(a), None) == EINVAL

    cur, mc, mr = np.array([0, 1], np.int32), np.array([0, 1, 1], np.int32), np.array([5, 6, 7], np.int32)
    out, r = np.zeros((8, 4)), _lib.BcResult()

    def correct(n=8, d=4, ld=4, sigma=150.0, cur=cur, mc=mc, mr=mr, n_cur=2, n_mnn=3, n_steps=1, x=x, out=out, args=True, result=True, steps=True, **seams):
        st = (_lib.BcStep * 1)(_lib.BcStep(cur_rows=_lib.ptr(cur), mnn_cur=_lib.ptr(mc), mnn_ref=_lib.ptr(mr), n_cur=n_cur, n_mnn=n_mnn))
        a = _lib.BcArgs(**seams)
        return L.crgpu_batch_correct_dev(None, _lib.ptr(x), n, d, ld, sigma, st if steps else None, n_steps, _lib.ptr(out), C.byref(a) if args else None,
                                         C.byref(r) if result else None)

    assert correct() == EINVAL              # NULL context, everything else in order
    bad_value = x.copy()
    bad_value[3, 1] = np.inf
    for kw in (dict(d=129, ld=129), dict(d=0), dict(ld=3), dict(n=0), dict(n=1 << 31), dict(sigma=-1.0), dict(sigma=float("nan")), dict(sigma=float("inf")),
               dict(x=bad_value), dict(cur=np.array([0, 8], np.int32)), dict(cur=np.array([0, -1], np.int32)), dict(cur=np.array([1, 1], np.int32)),
               dict(mc=np.array([0, 1, 8], np.int32)), dict(mr=np.array([5, -2, 7], np.int32)), dict(n_mnn=0), dict(n_cur=0), dict(x=None), dict(out=None),
               dict(args=False), dict(result=False), dict(steps=False), dict(cur=None), dict(mc=None), dict(mr=None), dict(row_tile=8), dict(pair_tile=12),
               dict(pair_tile=72), dict(slab_rows=40), dict(reserved=1)):
        assert correct(**kw) == EINVAL, kw
