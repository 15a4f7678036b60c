"""CPU-side checks of the MEASURE_PERTURBATIONS entry points (no GPU): the symbols are declared, exported, bound and written into
INTEGRATION.md; the two structs have one layout in the header, the library (crgpu_abi_layout), the ctypes table, the Rust blocks of
INTEGRATION.md and include/crgpu.hpp; the ABI version is still 3; the header states the stream, the bias, the quirk of the size factors
and what is not covered, and its three earlier "NOT covered: MEASURE_PERTURBATIONS" notes are gone; every refusal that needs no device
(the refusals that read the plan -- a gene or a group out of range, a group on both sides, too many bootstraps, too many LDS cells --
need a plan, which needs a device: tests/test_gpu_perturbations.py holds them with their messages); crgpu_perturbation_ci against
numpy on hand vectors, B = 1 and ties among them."""
import ctypes as C
import re

import numpy as np
import pytest

import perturbations_numpy as P
import test_abi_and_host as A
import test_subsample_abi as SA

ROOT = A.ROOT
NEW_SYMBOLS = ["crgpu_sseq_pair_bootstrap_dev", "crgpu_perturbation_ci"]
EINVAL = -1
STRUCTS = {"crgpu_pb_item": ("PbItem", "CrgpuPbItem", 16, 4), "crgpu_pb_args": ("PbArgs", "CrgpuPbArgs", 24, 8)}


@pytest.fixture(scope="module", autouse=True)
def built_library():
    from cellranger_amd import build

    build.build()


def _read(*parts):
    import os

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
    assert "getenv" not in _read("cellranger_amd", "csrc", "perturbations.h")      # every seam is an argument
    assert '#include "perturbations.h"' in _read("cellranger_amd", "csrc", "matrix_stages.hip")


def test_documents_describe_the_stage_and_its_deviations():
    hdr = _read("include", "crgpu.h")
    sec = hdr[hdr.index("---- MEASURE_PERTURBATIONS:"):]
    sec = sec[:sec.index("int crgpu_perturbation_ci(")]
    for phrase in ("measure_perturbations/__init__.py", "crispr/measure_perturbations.py", ":504-540", "measure_perturbations.py:527-528", "NOT", "reproduced",
                   "__umul64hi(w, n)", "n / 2^64", "EACH SIDE IS ONE GROUP", "ORIGINAL", "SORTED", "NOT covered:", "H5 writer", "random_raw()",
                   "(1 + (q >> 2), s, 0, 0)", "((uint64)stream << 33) | ((uint64)z << 32) | b", "pure function"):
        assert phrase in sec, phrase
    # the three earlier notes
    assert "built on them; MEASURE_PERTURBATIONS;" not in hdr and "the MEASURE_PERTURBATIONS stage itself" not in hdr
    assert "NOT covered: get_local_sseq_params" in hdr and "runs that test per perturbation" in hdr
    integ = _read("INTEGRATION.md")
    for phrase in ("MEASURE_PERTURBATIONS", "NOT reproduced", "SORTED order", "no H5 writer", "ONE group"):
        assert phrase in integ, phrase
    design, readme = _read("DESIGN.md"), _read("README.md")
    assert "k_pb_gather" in design and "k_pb_draws" in design and "perturbations.h" in design
    assert "measure_perturbations" in readme and "MEASURE_PERTURBATIONS" in readme and "reads these 32" in readme
    hpp = _read("include", "crgpu.hpp")
    assert "crgpu_sseq_pair_bootstrap_dev" in hpp and "crgpu_perturbation_ci" in hpp


@pytest.mark.parametrize("name", sorted(STRUCTS))
def test_struct_layout_agrees_everywhere(name):
    from cellranger_amd import _lib

    cls_name, rust_name, expect, expect_align = STRUCTS[name]
    size, align, fields = SA._header_struct(name)
    assert (size, align) == (expect, expect_align)
    lsize, lalign, lfields = A.library_layout(name)
    assert (size, align) == (lsize, lalign)
    assert [(o, s) for _, o, s in fields] == lfields
    cls = getattr(_lib, cls_name)
    assert C.sizeof(cls) == size
    assert [(f[0], getattr(cls, f[0]).offset, getattr(cls, f[0]).size) for f in cls._fields_] == fields
    assert SA._rust_struct(name, rust_name) == (size, align, fields)
    assert re.search(r"static_assert\(sizeof\(%s\) == %d\b" % (name, size), _read("include", "crgpu.hpp"))


def test_struct_offsets_by_hand():
    from cellranger_amd import _lib

    assert [(n, getattr(_lib.PbItem, n).offset) for n, _ in _lib.PbItem._fields_] == [("gene", 0), ("group_a", 4), ("group_b", 8), ("stream", 12)]
    assert [(n, getattr(_lib.PbArgs, n).offset) for n, _ in _lib.PbArgs._fields_] == [("n_bootstraps", 0), ("lds_cells", 4), ("draws_per_wg", 8), ("reserved", 12),
                                                                                    ("seed", 16)]


def test_entry_points_refuse_what_needs_no_device():
    from cellranger_amd import _lib

    L = _lib.load()
    Pt = _lib.ptr
    items = np.array([[0, 0, 1, 0]], np.uint32)
    a = _lib.PbArgs()
    sa, sb = np.zeros(500, np.uint64), np.zeros(500, np.uint64)
    fake = C.c_void_p(8)      # never read: a NULL argument and n_items == 0 are refused first
    good = (fake, fake, Pt(items), C.byref(a), Pt(sa), Pt(sb))
    for hole in range(6):
        args = [None if i == hole else g for i, g in enumerate(good)]
        assert L.crgpu_sseq_pair_bootstrap_dev(args[0], args[1], args[2], 1, args[3], args[4], args[5]) == EINVAL, hole
    assert L.crgpu_sseq_pair_bootstrap_dev(fake, fake, Pt(items), 0, C.byref(a), Pt(sa), Pt(sb)) == EINVAL      # n_items == 0
    # crgpu_perturbation_ci
    A_, B_ = np.array([3, 1], np.uint64), np.array([1, 1], np.uint64)
    fc, lo, hi = np.zeros(2), C.c_double(), C.c_double()

    def ci(a=Pt(A_), b=Pt(B_), n=2, s_a=1.0, s_b=1.0, lower=5.0, upper=95.0, out=Pt(fc), plo=C.byref(lo), phi=C.byref(hi)):
        return L.crgpu_perturbation_ci(a, b, n, s_a, s_b, lower, upper, out, plo, phi)

    assert ci() == 0 and ci(out=None) == 0
    assert ci(a=None) == EINVAL and ci(b=None) == EINVAL and ci(plo=None) == EINVAL and ci(phi=None) == EINVAL
    assert ci(n=0) == EINVAL and ci(n=65537) == EINVAL
    assert ci(s_a=-0.5) == EINVAL and ci(s_b=float("nan")) == EINVAL and ci(s_a=float("inf")) == EINVAL
    assert ci(lower=-1.0) == EINVAL and ci(upper=100.5) == EINVAL and ci(lower=float("nan")) == EINVAL


def _want(sa, sb, s_a, s_b, lower, upper):
    ta, tb = P.log_terms(sa, sb, s_a, s_b)
    return P.ci(sa, sb, s_a, s_b, lower, upper), ta, tb


@pytest.mark.parametrize("case", ["one_draw", "ties", "hand", "random_500", "zeros", "large"])
def test_perturbation_ci_against_numpy(case):
    """Per draw two divisions, two log2 and a subtraction, then the percentile's interpolation (a subtraction, a product, an addition of
    values no larger than the terms): each at most 1 ulp of a value bounded by max(1, |t_a|, |t_b|), together well inside 2^-50 of that
    bound.  With ties the two neighbours of the virtual index are equal and the interpolation is exact."""
    from cellranger_amd import engine as E

    rs = np.random.RandomState(3)
    sa, sb, s_a, s_b, lower, upper = {
        "one_draw": ([7], [2], 3.5, 11.25, 5.0, 95.0),
        "ties": ([4, 4, 4, 4, 9, 9, 9, 9, 9, 9], [2, 2, 2, 2, 2, 2, 2, 2, 2, 2], 10.0, 20.0, 5.0, 95.0),
        "hand": ([3, 1, 0, 7], [1, 1, 3, 0], 1.0, 3.0, 5.0, 95.0),
        "random_500": (rs.randint(0, 400, 500), rs.randint(100, 9000, 500), 97.3, 1290.1, 5.0, 95.0),
        "zeros": ([0, 0, 0], [0, 0, 0], 0.0, 0.0, 0.0, 100.0),
        "large": (rs.randint(2**40, 2**41, 64), rs.randint(0, 3, 64), 1e6, 0.5, 2.5, 97.5),
    }[case]
    lo, hi, fc = E.perturbation_ci(sa, sb, s_a, s_b, lower, upper)
    (wlo, whi, wfc), ta, tb = _want(sa, sb, s_a, s_b, lower, upper)
    tol = 2.0 ** -50 * max(1.0, np.abs(ta).max(), np.abs(tb).max())
    assert len(fc) == len(wfc) and np.abs(fc - wfc).max() <= tol and abs(lo - wlo) <= tol and abs(hi - whi) <= tol
    assert lo <= hi and fc.min() <= lo and hi <= fc.max()
    if case == "one_draw":
        assert lo == hi == fc[0]
    if case == "ties":
        assert lo == fc[0] and hi == fc[-1] and len(set(fc.tolist())) == 2
    if case == "zeros":
        assert lo == hi == 0.0
