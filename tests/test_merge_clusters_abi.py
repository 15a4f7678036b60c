"""CPU-side checks of the MERGE_CLUSTERS entry points (no GPU): the symbols are declared, exported, bound and written into INTEGRATION.md;
the two structs have one layout in the header, the library (crgpu_abi_layout), the ctypes table, the Rust blocks of INTEGRATION.md and
include/crgpu.hpp; the ABI version is still 3; the two new source files hold no getenv and README still says "reads these 32"; the
documents keep what other tests quote and name the deviation in cell order; every refusal that needs no device; crgpu_linkage_complete
equals the golden file's Z bit for bit on every iteration of every fixture, and K = 2, K = 1 (refused) and the tie rule by hand."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import merge_clusters_numpy as M
import test_abi_and_host as A
import test_subsample_abi as SA

ROOT = A.ROOT
NEW_SYMBOLS = ["crgpu_sseq_pairs_create_dev", "crgpu_sseq_pairs_free", "crgpu_sseq_pair_dev", "crgpu_cluster_medians_dev", "crgpu_linkage_complete"]
EINVAL = -1
STRUCTS = {"crgpu_sseq_pair_args": ("SseqPairArgs", "CrgpuSseqPairArgs", 24), "crgpu_sseq_pair_result": ("SseqPairResult", "CrgpuSseqPairResult", 224)}
GOLDEN = os.path.join(ROOT, "tests", "golden", "merge_clusters_reference.npz")


@pytest.fixture(scope="module", autouse=True)
def built_library():
    from cellranger_amd import build

    build.build()


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_new_symbols_are_declared_exported_and_bound():
    from cellranger_amd import _lib

    declared = A.header_symbols()
    L = C.CDLL(_lib.LIB_PATH)
    text = _read("INTEGRATION.md")
    for s in NEW_SYMBOLS:
        assert s in declared and hasattr(L, s) and s in _lib.SYMBOLS, s
        assert re.search(r"pub fn %s\(" % s, text), s
    assert _lib.load().crgpu_abi_version() == 3      # additive: no bump
    for src in ("sseq_pair.h", "merge_clusters.hip"):
        assert "getenv" not in _read("cellranger_amd", "csrc", src), src      # every seam is an argument
    assert "reads these 32" in _read("README.md")


def test_documents_describe_the_stage_and_keep_what_is_quoted():
    hdr = _read("include", "crgpu.h")
    assert "NOT covered: get_local_sseq_params" in hdr and "merge_clusters/__init__.py" in hdr and "graph_clustering.rs:156" in hdr
    assert "diffexp.py:69-85" in hdr and "ORDER OF THE CELLS" in hdr and "(height, id0, id1)" in hdr
    louvain = hdr[hdr.index("RUN_GRAPH_CLUSTERING: Louvain"):]
    assert re.search(r"NOT covered:[^/]*MERGE_CLUSTERS", louvain)
    readme = _read("README.md")
    for phrase in ("MERGE_CLUSTERS", "SNN similarity", "reads these 32", "merge_clusters", "(group, cell)"):
        assert phrase in readme, phrase
    assert "k_sq_pair_row_sums" in _read("DESIGN.md") and "k_mc_median" in _read("DESIGN.md")


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
    assert re.search(r"static_assert\(sizeof\(%s\) == %d\b" % (name, size), _read("include", "crgpu.hpp"))


def test_entry_points_refuse_what_needs_no_device():
    from cellranger_amd import _lib

    L = _lib.load()
    m = _lib.MatrixDevView()
    m.n_barcodes, m.nnz = 4, 6
    a = _lib.SseqPairArgs(n_features=3)
    out = C.c_void_p()
    res = _lib.SseqPairResult()
    grp = np.array([0, 1, 0, 1], np.int32)
    ga, gb = np.array([0], np.uint32), np.array([1], np.uint32)
    fake = C.c_void_p(8)      # never read: a NULL argument is refused first
    P = _lib.ptr
    for args in ((None, C.byref(m), P(grp), C.byref(a), C.byref(out)), (fake, None, P(grp), C.byref(a), C.byref(out)),
                 (fake, C.byref(m), None, C.byref(a), C.byref(out)), (fake, C.byref(m), P(grp), None, C.byref(out)),
                 (fake, C.byref(m), P(grp), C.byref(a), None)):
        assert L.crgpu_sseq_pairs_create_dev(args[0], args[1], args[2], 2, args[3], args[4]) == EINVAL
    assert not out.value
    for args in ((None, fake, P(ga), P(gb), C.byref(a), C.byref(res)), (fake, None, P(ga), P(gb), C.byref(a), C.byref(res)),
                 (fake, fake, None, P(gb), C.byref(a), C.byref(res)), (fake, fake, P(ga), None, C.byref(a), C.byref(res)),
                 (fake, fake, P(ga), P(gb), None, C.byref(res)), (fake, fake, P(ga), P(gb), C.byref(a), None)):
        assert L.crgpu_sseq_pair_dev(args[0], args[1], args[2], 1, args[3], 1, args[4], args[5]) == EINVAL
    L.crgpu_sseq_pairs_free(None, None)      # a no-op
    x, lab, med = np.zeros((4, 2)), np.zeros(4, np.int32), np.zeros((1, 2))
    assert L.crgpu_cluster_medians_dev(None, P(x), 4, 2, 2, P(lab), 1, P(med), None) == EINVAL
    assert L.crgpu_cluster_medians_dev(fake, None, 4, 2, 2, P(lab), 1, P(med), None) == EINVAL
    assert L.crgpu_cluster_medians_dev(fake, P(x), 4, 2, 2, None, 1, P(med), None) == EINVAL
    assert L.crgpu_cluster_medians_dev(fake, P(x), 4, 2, 2, P(lab), 1, None, None) == EINVAL
    # the host-only linkage: NULLs, K = 1, K above the limit, d = 0, a value that is not finite
    pts, z = np.array([[0.0], [1.0]]), np.zeros((1, 4))
    assert L.crgpu_linkage_complete(None, 2, 1, P(z)) == EINVAL and L.crgpu_linkage_complete(P(pts), 2, 1, None) == EINVAL
    assert L.crgpu_linkage_complete(P(pts), 1, 1, P(z)) == EINVAL and L.crgpu_linkage_complete(P(pts), 2, 0, P(z)) == EINVAL
    assert L.crgpu_linkage_complete(P(pts), _lib.SSEQ_MAX_K + 1, 1, P(z)) == EINVAL
    assert L.crgpu_linkage_complete(P(np.array([[0.0], [np.inf]])), 2, 1, P(z)) == EINVAL and L.crgpu_linkage_complete(P(np.array([[np.nan], [0.0]])), 2, 1, P(z)) == EINVAL
    assert L.crgpu_linkage_complete(P(pts), 2, 1, P(z)) == 0 and z.tolist() == [[0.0, 1.0, 1.0, 2.0]]


def test_linkage_equals_the_file_bit_for_bit():
    from cellranger_amd import engine as E

    ref = np.load(GOLDEN)
    n = 0
    for name in sorted(M.FIXTURES):
        for i in range(int(ref[name + ".counts"][3])):
            Z = E.linkage_complete(ref["%s.medoids.%d" % (name, i)])
            assert Z.tobytes() == ref["%s.Z.%d" % (name, i)].tobytes(), (name, i)
            n += 1
    assert n >= 20


def test_linkage_hand_cases_and_the_tie_rule():
    from cellranger_amd import engine as E

    assert E.linkage_complete([[0.0, 0.0], [3.0, 4.0]]).tolist() == [[0.0, 1.0, 5.0, 2.0]]      # K = 2
    with pytest.raises(ValueError):
        E.linkage_complete([[1.0, 2.0]])      # K = 1
    assert E.linkage_complete([[0.0], [1.0], [3.0]]).tolist() == [[0.0, 1.0, 1.0, 2.0], [2.0, 3.0, 3.0, 3.0]]
    # three distances of 1: the smallest (height, id0, id1) first, and the restatement has the same rule
    pts = np.array([[0.0], [1.0], [2.0], [3.0]])
    assert E.linkage_complete(pts).tolist() == [[0.0, 1.0, 1.0, 2.0], [2.0, 3.0, 1.0, 2.0], [4.0, 5.0, 3.0, 4.0]]
    rs = np.random.RandomState(11)
    for K, d in ((2, 1), (3, 2), (17, 5), (64, 3), (200, 10)):
        pts = rs.randint(0, 4, (K, d)).astype(np.float64) if K <= 64 else rs.normal(0, 1, (K, d))      # small integers: many ties
        assert E.linkage_complete(pts).tobytes() == M.linkage_complete(pts).tobytes(), (K, d)
