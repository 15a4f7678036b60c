"""CPU-side checks of the RUN_PCA entry points (no GPU): the symbols are declared, exported, bound and written into INTEGRATION.md; the two
structs have one layout in the header, the library (crgpu_abi_layout), the ctypes table, the Rust blocks of INTEGRATION.md and
include/crgpu.hpp; the ABI version is still 3; the seams are fields, so the README still says the library "reads these 32" environment
variables; crgpu_pca_dev refuses every bad argument with a NULL context.  The three host functions against what they restate:
crgpu_legacy_randn equals np.random.RandomState(seed).randn(n) bit for bit; crgpu_normalized_dispersion is bit-equal to the reference's
get_normalized_dispersion as recorded in tests/golden/pca_reference.npz (NaN places and the signs of the infinities included);
crgpu_small_svd on the recorded B matrices of a first Lanczos pass and of a restarted one (with its full column k)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pca_numpy as P
import test_abi_and_host as A
import test_subsample_abi as SA

ROOT = A.ROOT
NEW_SYMBOLS = ["crgpu_pca_dev", "crgpu_legacy_randn", "crgpu_normalized_dispersion", "crgpu_small_svd"]
EINVAL = -1
STRUCTS = {"crgpu_pca_args": ("PcaArgs", "CrgpuPcaArgs", 64), "crgpu_pca_result": ("PcaResult", "CrgpuPcaResult", 128)}
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "pca_reference.npz"))
EPS = np.finfo(np.float64).eps


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
    consts = dict(re.findall(r"#define (CRGPU_PCA_\w+) (\d+)", hdr))
    assert [int(consts[k]) for k in ("CRGPU_PCA_MAX_COMPONENTS", "CRGPU_PCA_DEFAULT_THRESHOLD", "CRGPU_PCA_OK", "CRGPU_PCA_NULL_AXIS", "CRGPU_PCA_RANK_TOO_SMALL")] \
        == [_lib.PCA_MAX_COMPONENTS, _lib.PCA_DEFAULT_THRESHOLD, _lib.PCA_OK, _lib.PCA_NULL_AXIS, _lib.PCA_RANK_TOO_SMALL] == [128, 2, 0, 1, 2]
    section = hdr[hdr.index("---- RUN_PCA:"):hdr.index("#define CRGPU_PCA_MAX_COMPONENTS")]
    for cited in ("analysis/pca.py:49-209", "analysis/irlb.py:61-231", "analysis/stats.py", "matrix.py:788-810", "1.7.2", "ZERO-COUNT BARCODE", "START VECTOR NORM",
                  "THRESHOLD ORDER", "SIGN OF A COMPONENT", "Not covered by this stage", "pca_bcs", "H5 and CSV", "split()", "float32", "normalize_by_idf"):
        assert cited in section, cited
    with open(os.path.join(ROOT, "README.md")) as f:
        readme = f.read()
    assert "reads these 32" in readme and "crgpu_pca_dev" in readme
    with open(os.path.join(ROOT, "cellranger_amd", "csrc", "pca.hip")) as f:
        src = f.read()
    assert "getenv" not in src and "atomicAdd(counts + r, (unsigned long long)" in src      # the seams are fields; the only atomic adds integers
    assert not re.search(r"atomicAdd\([^)]*double", src)


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
    view = _lib.MatrixDevView()
    res = _lib.PcaResult()
    idx, start = np.array([0, 1], dtype=np.uint64), np.ones(4)
    good = dict(n_components=3)
    # a NULL context first, everything else in order; then every bad argument, which gives the same code without a context
    for fields in (good, dict(n_components=0), dict(n_components=129), dict(n_components=3, wave_block=100), dict(n_components=3, dot_parts_per_block=65),
                   dict(n_components=3, reserved0=1), dict(n_components=3, reserved1=1), dict(n_components=3, pca_bc_indices=_lib.ptr(idx)),
                   dict(n_components=3, n_pca_bcs=2), dict(n_components=3, start=_lib.ptr(start)), dict(n_components=3, n_start=4)):
        a = _lib.PcaArgs(**fields)
        assert L.crgpu_pca_dev(None, C.byref(view), 10, C.byref(a), C.byref(res)) == EINVAL, fields
    a = _lib.PcaArgs(**good)
    assert L.crgpu_pca_dev(None, None, 10, C.byref(a), C.byref(res)) == EINVAL
    assert L.crgpu_pca_dev(None, C.byref(view), 10, None, C.byref(res)) == EINVAL
    assert L.crgpu_pca_dev(None, C.byref(view), 10, C.byref(a), None) == EINVAL
    out = np.zeros(4)
    assert L.crgpu_legacy_randn(0, 4, None) == EINVAL and L.crgpu_legacy_randn(0, 0, None) == 0
    for args in ((None, _lib.ptr(out), 4, 20, _lib.ptr(out)), (_lib.ptr(out), None, 4, 20, _lib.ptr(out)), (_lib.ptr(out), _lib.ptr(out), 4, 20, None),
                 (_lib.ptr(out), _lib.ptr(out), 0, 20, _lib.ptr(out)), (_lib.ptr(out), _lib.ptr(out), 4, 0, _lib.ptr(out)),
                 (_lib.ptr(out), _lib.ptr(out), 4, 101, _lib.ptr(out))):
        assert L.crgpu_normalized_dispersion(*args) == EINVAL
    nan_mu = np.array([1.0, np.nan, 2.0, 3.0])
    assert L.crgpu_normalized_dispersion(_lib.ptr(nan_mu), _lib.ptr(out), 4, 20, _lib.ptr(out)) == EINVAL
    b = np.eye(3)
    u, s, vt = np.zeros((3, 3)), np.zeros(3), np.zeros((3, 3))
    assert L.crgpu_small_svd(None, 3, _lib.ptr(u), _lib.ptr(s), _lib.ptr(vt)) == EINVAL
    assert L.crgpu_small_svd(_lib.ptr(b), 0, _lib.ptr(u), _lib.ptr(s), _lib.ptr(vt)) == EINVAL
    assert L.crgpu_small_svd(_lib.ptr(b), 149, _lib.ptr(u), _lib.ptr(s), _lib.ptr(vt)) == EINVAL
    b[1, 1] = np.inf
    assert L.crgpu_small_svd(_lib.ptr(b), 3, _lib.ptr(u), _lib.ptr(s), _lib.ptr(vt)) == EINVAL


@pytest.mark.parametrize("seed", [0, 1, 2 ** 31 + 5])
def test_legacy_randn_is_numpys_bit_for_bit(seed):
    from cellranger_amd import engine as E

    for n in (1, 2, 3, 624, 625, 36601):      # an odd n leaves the second value of a pair cached and unused
        got, ref = E.legacy_randn(seed, n), np.random.RandomState(seed).randn(n)
        assert np.array_equal(got.view(np.uint64), ref.view(np.uint64)), (seed, n)


def _same_bits_or_nan(got, ref):
    return np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(got[~np.isnan(ref)].view(np.uint64), ref[~np.isnan(ref)].view(np.uint64))


@pytest.mark.parametrize("name", sorted(P.FIXTURES))
def test_normalized_dispersion_is_the_references_bit_for_bit(name):
    from cellranger_amd import engine as E

    mu, var, ref = GOLD[name + "_mu"], GOLD[name + "_var"], GOLD[name + "_disp_thr"]
    got = E.normalized_dispersion(mu, var)
    assert _same_bits_or_nan(got, ref)      # the signs of the infinities are bits too
    assert np.array_equal(np.argsort(got, kind="stable"), np.argsort(ref, kind="stable"))


def test_normalized_dispersion_pathological_fixtures_are_what_they_claim():
    mad0, equal, var0 = GOLD["mad0_disp_thr"], GOLD["equal_mu"], GOLD["var0_var"]
    assert np.isnan(mad0).sum() >= 40 and np.isinf(mad0).any()      # a bin whose MAD is 0: 0 / 0 and x / 0
    assert len(np.unique(equal)) == 1                                # all means equal: the early return
    assert np.array_equal(GOLD["equal_disp_thr"], (GOLD["equal_var"] - equal) / np.square(equal))
    assert var0[-1] == 0.0      # the feature that holds 3 in every cell of equal depth: variance exactly 0
    assert not np.array_equal(GOLD["thr_features_selected"], np.arange(len(GOLD["thr_features_selected"])))      # org_cols_used is no identity
    assert int(GOLD["small_retried"]) == 1 and int(GOLD["small_n_components"]) == 6


RECORDED_B = [k for k in GOLD.files if re.fullmatch(r"\w+_B[01]", k)]


@pytest.mark.parametrize("key", sorted(RECORDED_B))
def test_small_svd_on_the_recorded_b_matrices(key):
    from cellranger_amd import engine as E

    b = GOLD[key]
    n = len(b)
    if key.endswith("_B1"):      # a restarted B: a diagonal block and a full column k
        k = int(np.flatnonzero(np.count_nonzero(b, axis=0) > 2)[0])
        assert k >= 1 and np.count_nonzero(b[:k, :k] - np.diag(np.diag(b[:k, :k]))) == 0 and np.count_nonzero(b[:k, k]) > 2
    u, s, vt = E.small_svd(b)
    ref = np.linalg.svd(b, compute_uv=False)
    norm = ref[0]      # ||B||
    assert (np.diff(s) <= 0).all()
    assert np.abs(s - ref).max() <= 8 * EPS * norm
    assert np.abs((u * s) @ vt - b).max() <= 8 * EPS * norm
    assert np.abs(u.T @ u - np.eye(n)).max() <= 1e-14 and np.abs(vt @ vt.T - np.eye(n)).max() <= 1e-14


def test_small_svd_of_a_singular_matrix_completes_u():
    from cellranger_amd import engine as E

    b = np.zeros((4, 4))
    b[0, 0], b[1, 1], b[0, 1] = 3.0, 2.0, 0.5
    u, s, vt = E.small_svd(b)
    assert s[2] == 0.0 and s[3] == 0.0
    assert np.abs((u * s) @ vt - b).max() <= 8 * EPS * 3.1 and np.abs(u.T @ u - np.eye(4)).max() <= 1e-14
