"""CPU-side checks of the Louvain entry points (no GPU): the symbols are declared, exported, bound and written into INTEGRATION.md; the
two structs have one layout in the header, the library (crgpu_abi_layout), the ctypes table, the Rust blocks of INTEGRATION.md and
include/crgpu.hpp; the ABI version is still 3; crgpu_modularity, which needs no device, gives the hand-computed S and M and equals the
restatement on every labelling tried; every refusal that needs no device comes back without a context; the seams are fields, so
louvain.hip holds no getenv and the README still says the library "reads these 32" environment variables."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import louvain_numpy as R
import test_abi_and_host as A
import test_subsample_abi as SA

ROOT = A.ROOT
NEW_SYMBOLS = ["crgpu_louvain_dev", "crgpu_modularity"]
EINVAL = -1
STRUCTS = {"crgpu_louvain_args": ("LouvainArgs", "CrgpuLouvainArgs", 32), "crgpu_louvain_result": ("LouvainResult", "CrgpuLouvainResult", 136)}


@pytest.fixture(scope="module", autouse=True)
def built_library():
    from cellranger_amd import build

    build.build()


def _erange():
    with open(os.path.join(ROOT, "include", "crgpu.h")) as f:
        return int(re.search(r"#define CRGPU_ERANGE \((-?\d+)\)", f.read()).group(1))


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
    assert int(re.search(r"#define CRGPU_LOUVAIN_MAX_LEVELS (\d+)", hdr).group(1)) == 64 == _lib.LOUVAIN_MAX_LEVELS == R.MAX_LEVELS
    section = hdr[hdr.index("---- RUN_GRAPH_CLUSTERING: Louvain"):hdr.index("#define CRGPU_LOUVAIN_MAX_LEVELS")]
    for cited in ("graphclust.py", "Blondel", "no parity with the binary", "THE SINGLETON RULE", "(G, C == own, -C)", "not verified against the binary",
                  "NOT covered", "MERGE_CLUSTERS", "SNN similarity"):
        assert cited in section, cited
    with open(os.path.join(ROOT, "README.md")) as f:
        readme = f.read()
    assert "reads these 32" in readme and "crgpu_louvain_dev" in readme and "bin/louvain" in readme
    assert "Louvain and `convert`" not in readme and "SNN similarity" in readme and "MERGE_CLUSTERS" in readme
    with open(os.path.join(ROOT, "cellranger_amd", "csrc", "louvain.hip")) as f:
        src = f.read()
    body = src[src.index("#include"):]
    assert "getenv" not in src and "hipGraph" not in src and "Cooperative" not in src
    assert not re.search(r"\b(float|expf?|logf?|sqrtf?|pow)\b", body)      # integers; double only carries the timings
    assert all("_ms" in line or "std::milli" in line for line in body.splitlines() if re.search(r"\bdouble\b", line))
    for name in ("louvain_pairs", "modularity", "louvain_labels", "run_graph_clustering"):
        assert hasattr(engine, name), name
    assert hasattr(engine.Context, "louvain")
    assert (_lib.LOUVAIN_MAX_ROUNDS, _lib.LOUVAIN_WAVE_DEG_MAX, _lib.LOUVAIN_LDS_DEG_MAX, _lib.LOUVAIN_BATCH) == tuple(
        int(re.search(r"#define %s (\d+)u" % k, src).group(1)) for k in ("LV_MAX_ROUNDS", "LV_WAVE_DEG_CAP", "LV_WG_DEG_CAP", "LV_BATCH"))


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


@pytest.mark.parametrize("name", sorted(R.hand_cases()))
def test_modularity_on_the_hand_cases(name):
    from cellranger_amd import engine

    n, edges, labels, s_m = R.hand_cases()[name]
    indptr, indices, w = R.csr_from_edges(n, edges)
    S, M, Q = engine.modularity(indptr, indices, labels)
    if s_m:
        assert (S, M) == s_m
    assert (S, M) == R.modularity_S((indptr, indices, w), labels) and Q == S / float(M) ** 2
    rs = np.random.RandomState(len(name))
    ww = rs.randint(1, 1000, len(edges))
    graph = R.csr_from_edges(n, edges, ww)
    for groups in (1, 2, n):
        c = rs.randint(0, groups, n)
        assert engine.modularity(graph[0], graph[1], c, weights=graph[2])[:2] == R.modularity_S(graph, c)
    assert engine.modularity(graph[0], graph[1], np.arange(n) * 1000, weights=graph[2])[:2] == R.modularity_S(graph, np.arange(n))


def test_modularity_near_the_limit_and_its_refusals():
    from cellranger_amd import _lib, engine

    ptr = _lib.ptr
    L = _lib.load()
    indptr, indices, w = R.csr_from_edges(4, [(0, 1), (1, 2), (2, 3), (0, 3)], [(1 << 28) - 1, 1 << 28, 1 << 28, 1 << 28])
    assert int(w.sum()) == (1 << 31) - 2
    for c in ([0, 0, 1, 1], [0, 1, 2, 3], [0, 0, 0, 0]):
        assert engine.modularity(indptr, indices, c, weights=w)[:2] == R.modularity_S((indptr, indices, w), c)
    S, M = C.c_int64(), C.c_int64()
    p, i, ww, lab = indptr.astype(np.int64), indices.astype(np.int32), w.astype(np.uint32), np.zeros(4, np.int32)

    def call(p=p, i=i, ww=ww, lab=lab, n=4):
        return L.crgpu_modularity(ptr(p), ptr(i), ptr(ww), n, ptr(lab), C.byref(S), C.byref(M))

    assert call() == 0
    over, zero, out_of_range, bad_ptr, neg = ww.copy(), ww.copy(), i.copy(), p.copy(), lab.copy()
    over[-1] += 2
    zero[0], out_of_range[1], bad_ptr[0], neg[2] = 0, 4, 1, -1
    assert call(ww=over) == _erange()
    for kw in (dict(ww=zero), dict(i=out_of_range), dict(p=bad_ptr), dict(lab=neg), dict(n=0), dict(n=1 << 31)):
        assert call(**kw) == EINVAL, kw
    assert L.crgpu_modularity(None, ptr(i), ptr(ww), 4, ptr(lab), C.byref(S), C.byref(M)) == EINVAL
    assert L.crgpu_modularity(ptr(p), ptr(i), ptr(ww), 4, None, C.byref(S), C.byref(M)) == EINVAL
    assert L.crgpu_modularity(ptr(p), ptr(i), ptr(ww), 4, ptr(lab), None, C.byref(M)) == EINVAL
    with pytest.raises(ValueError):
        engine.modularity(indptr, indices, [0, 0, 0])


def test_the_entry_point_refuses_without_a_context():
    """CRGPU_EINVAL comes first for the missing context, so each call below is also made in order and must give the same code -- what
    tells the refusals apart is the live context of tests/test_gpu_louvain.py."""
    from cellranger_amd import _lib

    L, ptr = _lib.load(), _lib.ptr
    indptr, indices, w = R.csr_from_edges(4, [(0, 1), (1, 2), (2, 3)])
    p, i, ww = indptr.astype(np.int64), indices.astype(np.int32), w.astype(np.uint32)
    res = _lib.LouvainResult()
    for args in (_lib.LouvainArgs(symmetrize=1), _lib.LouvainArgs(symmetrize=2), _lib.LouvainArgs(wave_deg_max=128), _lib.LouvainArgs(lds_deg_max=2048),
                 _lib.LouvainArgs(reserved0=1)):
        assert L.crgpu_louvain_dev(None, ptr(p), ptr(i), ptr(ww), 4, C.byref(args), C.byref(res)) == EINVAL
    a = _lib.LouvainArgs()
    assert L.crgpu_louvain_dev(None, None, ptr(i), ptr(ww), 4, C.byref(a), C.byref(res)) == EINVAL
    assert L.crgpu_louvain_dev(None, ptr(p), ptr(i), ptr(ww), 4, None, C.byref(res)) == EINVAL
    assert L.crgpu_louvain_dev(None, ptr(p), ptr(i), ptr(ww), 4, C.byref(a), None) == EINVAL


def test_pairs_give_the_level_zero_labels():
    """engine.louvain_pairs on a result of the restatement's form: load_louvain_results' rule keeps the level-0 line of every node"""
    from cellranger_amd import engine

    indptr, indices = R.golden_fixtures()["groups_s2_k15"]
    r = R.louvain(indptr, indices)
    assert len(r["levels"]) >= 2
    pairs = engine.louvain_pairs(r)
    assert pairs == R.pairs(r) and len(pairs) == sum(r["nodes"])
    use = np.arange(300) * 2
    labels = engine.louvain_labels(600, use, pairs)
    assert np.array_equal(labels[use], 1 + r["level0"]) and not labels[use + 1].any()
    with pytest.raises(ValueError, match="device"):
        engine.run_graph_clustering(None, np.zeros((10, 2)), louvain="host")
