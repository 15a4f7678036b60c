"""CPU-side checks of the sSeq entry points (no GPU): the symbols are declared, exported, bound and written into INTEGRATION.md; the three
structs have one layout in the header, the library (crgpu_abi_layout), the ctypes table, the Rust blocks of INTEGRATION.md and
include/crgpu.hpp; the ABI version is still 3; the header, README and DESIGN.md say that the diff_exp crate's source was not available;
every entry point refuses a NULL context or argument, and without a device G < 3, N < 2, K < 2, a label outside 1 .. K, an empty
cluster (with a live context, and the message: tests/test_gpu_sseq.py); crgpu_sseq_adjust_bh equals the restatement, ties and n = 1
included; the feature adds no environment switch."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import sseq_numpy as R
import test_abi_and_host as A
import test_subsample_abi as SA

ROOT = A.ROOT
NEW_SYMBOLS = ["crgpu_sseq_params_dev", "crgpu_sseq_params_free", "crgpu_sseq_params_get", "crgpu_sseq_diffexp_dev", "crgpu_sseq_adjust_bh"]
EINVAL = -1
STRUCTS = {"crgpu_sseq_args": ("SseqArgs", "CrgpuSseqArgs", 16), "crgpu_sseq_params_info": ("SseqParamsInfo", "CrgpuSseqParamsInfo", 80),
           "crgpu_sseq_result": ("SseqResult", "CrgpuSseqResult", 160)}


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
    assert int(re.search(r"#define CRGPU_SSEQ_MAX_K (\d+)", hdr).group(1)) == _lib.SSEQ_MAX_K and _lib.SSEQ_BIG_COUNT == R.BIG_COUNT == 900
    assert "WHOSE SOURCE WAS NOT AVAILABLE" in hdr and "No parity with the crate" in hdr and "NOT covered: get_local_sseq_params" in hdr
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        with open(os.path.join(ROOT, doc)) as f:
            t = f.read()
        assert "diff_exp" in t and "not available" in t, doc
    with open(os.path.join(ROOT, "README.md")) as f:
        assert "reads these 32" in f.read()
    with open(os.path.join(ROOT, "cellranger_amd", "csrc", "sseq.h")) as f:
        assert "getenv" not in f.read()      # the class thresholds are arguments, not switches


@pytest.mark.parametrize("name", sorted(STRUCTS))
def test_struct_layout_agrees_everywhere(name):
    from cellranger_amd import _lib

    cls_name, rust_name, expect = STRUCTS[name]
    size, align, fields = SA._header_struct(name)
    assert (size, align) == (expect, 8 if name != "crgpu_sseq_args" else 4)
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
    m = _lib.MatrixDevView()
    m.n_barcodes, m.nnz = 4, 6
    a = _lib.SseqArgs(n_features=3)
    out = C.c_void_p()
    res = _lib.SseqResult()
    info = _lib.SseqParamsInfo()
    lab = np.array([1, 2, 1, 2], np.int32)
    fake = C.c_void_p(8)      # never read: the NULL context is refused first
    assert L.crgpu_sseq_params_dev(None, C.byref(m), C.byref(a), C.byref(out)) == EINVAL and not out.value
    assert L.crgpu_sseq_params_dev(fake, None, C.byref(a), C.byref(out)) == EINVAL
    assert L.crgpu_sseq_params_dev(fake, C.byref(m), None, C.byref(out)) == EINVAL
    assert L.crgpu_sseq_params_dev(fake, C.byref(m), C.byref(a), None) == EINVAL
    assert L.crgpu_sseq_params_get(None, fake, C.byref(info)) == EINVAL and L.crgpu_sseq_params_get(fake, None, C.byref(info)) == EINVAL
    assert L.crgpu_sseq_params_get(fake, fake, None) == EINVAL
    for ctx, mm, pp, ll, aa, rr in ((None, C.byref(m), fake, _lib.ptr(lab), C.byref(a), C.byref(res)), (fake, None, fake, _lib.ptr(lab), C.byref(a), C.byref(res)),
                                    (fake, C.byref(m), None, _lib.ptr(lab), C.byref(a), C.byref(res)), (fake, C.byref(m), fake, None, C.byref(a), C.byref(res)),
                                    (fake, C.byref(m), fake, _lib.ptr(lab), None, C.byref(res)), (fake, C.byref(m), fake, _lib.ptr(lab), C.byref(a), None)):
        assert L.crgpu_sseq_diffexp_dev(ctx, mm, pp, ll, 2, aa, rr) == EINVAL
    # G < 3, N < 2, K < 2, a label outside 1 .. K, an empty cluster: the same code without a context
    for G, N, K, labels in ((2, 4, 2, [1, 2, 1, 2]), (3, 1, 2, [1]), (3, 4, 1, [1, 1, 1, 1]), (3, 4, 2, [1, 2, 3, 1]), (3, 4, 2, [0, 1, 2, 1]), (3, 4, 3, [1, 2, 1, 2])):
        m.n_barcodes, a.n_features = N, G
        assert L.crgpu_sseq_params_dev(None, C.byref(m), C.byref(a), C.byref(out)) == EINVAL
        assert L.crgpu_sseq_diffexp_dev(None, C.byref(m), fake, _lib.ptr(np.array(labels, np.int32)), K, C.byref(a), C.byref(res)) == EINVAL
    L.crgpu_sseq_params_free(None, None)      # a no-op
    q = np.zeros(2)
    assert L.crgpu_sseq_adjust_bh(None, 2, _lib.ptr(q)) == EINVAL and L.crgpu_sseq_adjust_bh(_lib.ptr(q), 2, None) == EINVAL
    assert L.crgpu_sseq_adjust_bh(None, 0, None) == 0


def test_adjust_bh_equals_the_restatement():
    from cellranger_amd import engine as E

    q = E.sseq_adjust_bh([0.01, 0.04, 0.04, 0.03, 0.5])
    assert np.array_equal(q, R.adjust_bh([0.01, 0.04, 0.04, 0.03, 0.5])) and q[1] == q[2] and abs(q[0] - 0.05) < 1e-16 and q[4] == 0.5
    assert E.sseq_adjust_bh([0.3]).tolist() == [0.3] and len(E.sseq_adjust_bh([])) == 0
    rs = np.random.RandomState(5)
    for n in (1, 2, 3, 17, 1000):
        p = rs.uniform(0, 1, n) ** 3
        p[rs.randint(0, n, n // 3)] = p[0]      # ties
        if n > 2:
            p[1] = 1.7      # an asymptotic p is not clipped
        assert np.array_equal(E.sseq_adjust_bh(p), R.adjust_bh(p)), n


def test_header_strings_of_the_csv():
    from cellranger_amd import engine as E

    assert E.differential_expression_header(2) == ["Feature ID", "Feature Name", "Cluster 1 Mean Counts", "Cluster 1 Log2 fold change", "Cluster 1 Adjusted p value",
                                                   "Cluster 2 Mean Counts", "Cluster 2 Log2 fold change", "Cluster 2 Adjusted p value"]
    assert E.differential_expression_header(1, ["KRAS"])[2:] == ["Perturbation KRAS, Mean Counts", "Perturbation KRAS, Log2 fold change",
                                                                 "Perturbation KRAS, Adjusted p value"]
