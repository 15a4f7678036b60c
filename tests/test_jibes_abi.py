"""CPU-side checks of the JIBES entry points (no GPU): the symbols are declared, exported, bound and written into INTEGRATION.md, the
device entry points refuse a NULL context, the three structs have one layout in the header, the library (crgpu_abi_layout), the ctypes
table, the Rust blocks of INTEGRATION.md and include/crgpu.hpp, and the host functions equal the restatement tests/jibes_numpy.py.

Equality where integers decide: the latent states, the flags, z.  The log prior and the expected cells go through the C library's
exp / log / lgamma where the restatement goes through Python's: each is within an ulp or two of the true value, the prior adds four
such terms of magnitude <= 40, so 1e-13 absolute is asserted for it; the root of the cell estimate inherits the 1e-13 relative
agreement of the Poisson counts and has slope about 1, so 1e-9 relative.  The initial parameters are numpy's pairwise sums restated in
C: the golden values (recorded from the reference) are met bit for bit, except the std, whose squares numpy takes through abs(x)^2 as
this does: within 2 ulp is asserted."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import jibes_numpy as R
import test_abi_and_host as A
import test_rtl_tags_abi as T
import test_subsample_abi as SA
from test_jibes_restatement import golden

ROOT = A.ROOT
NEW_SYMBOLS = ["crgpu_jibes_expected_cells", "crgpu_jibes_latent_states", "crgpu_jibes_log_prior", "crgpu_jibes_initial_parameters",
               "crgpu_jibes_tag_counts_dev", "crgpu_jibes_fit_dev"]
EINVAL, ERANGE = -1, -6
STRUCTS = {"crgpu_jibes_setup": ("JibesSetup", "CrgpuJibesSetup", 24, T), "crgpu_jibes_fit_args": ("JibesFitArgs", "CrgpuJibesFitArgs", 136, SA),
           "crgpu_jibes_fit_result": ("JibesFitResult", "CrgpuJibesFitResult", 416, T)}


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
    for macro, v in (("MAX_TAGS", 16), ("MAX_K_LETS", 3), ("MAX_STATES", 970), ("NEAR_ZERO", 12), ("CANT_CONVERGE", 1)):
        assert int(re.search(r"#define CRGPU_JIBES_%s (\d+)" % macro, hdr).group(1)) == v == getattr(_lib, "JIBES_" + macro)
    with open(os.path.join(ROOT, "README.md")) as f:
        assert "CRGPU_JIBES_BATCH" in f.read()


def test_device_entry_points_refuse_null():
    from cellranger_amd import _lib

    L = _lib.load()
    a, r = _lib.JibesFitArgs(), _lib.JibesFitResult()
    y = np.zeros((2, 2))
    assert L.crgpu_jibes_fit_dev(None, _lib.ptr(y), 2, 2, C.byref(a), C.byref(r)) == EINVAL
    rows = np.zeros(1, np.uint32)
    assert L.crgpu_jibes_tag_counts_dev(None, None, _lib.ptr(rows), 1, 4, None, None, None, None, None) == EINVAL
    assert L.crgpu_jibes_expected_cells(5, 2000, None) == EINVAL


@pytest.mark.parametrize("name", sorted(STRUCTS))
def test_struct_layout_agrees_everywhere(name):
    from cellranger_amd import _lib

    cls_name, rust_name, expect, parser = STRUCTS[name]
    size, align, fields = parser._header_struct(name)
    assert (size, align) == (expect, 8)
    lsize, lalign, lfields = A.library_layout(name)
    assert (size, align) == (lsize, lalign)
    assert [(o, s) for _, o, s in fields] == lfields
    cls = getattr(_lib, cls_name)
    assert C.sizeof(cls) == size
    assert [(f[0], getattr(cls, f[0]).offset, getattr(cls, f[0]).size) for f in cls._fields_] == fields
    assert parser._rust_struct(name, rust_name) == (size, align, fields)
    with open(os.path.join(ROOT, "include", "crgpu.hpp")) as f:
        hpp = f.read()
    assert re.search(r"static_assert\(sizeof\(%s\) == %d\b" % (name, size), hpp)


def test_latent_states_and_prior_equal_the_restatement():
    from cellranger_amd import engine as E

    cases = [(65, 2, 2000), (400, 3, 2000), (1000, 12, 4000), (130, 16, 300), (1, 3, 2000), (45, 3, 100), (40, 2, 100), (6, 4, 95000),
             (50000, 12, 95000), (5, 1, 2000), (300, 14, 500), (300, 15, 500)]
    for n, k, ng in cases:
        est = R.expected_total_cells(n, ng)
        got = E.jibes_expected_cells(n, ng)
        assert abs(got - est) <= 1e-9 * est, (n, ng, got, est)
        for mk in (3, 2, 1):
            states, limited, mm, mmk, _ = R.latent_state_setup(n, k, ng, mk, est)
            lat = E.jibes_latent_states(n, k, ng, mk, est)
            assert lat["states"].dtype == np.uint8 and np.array_equal(lat["states"], states), (n, k, ng, mk)
            assert (lat["k_let_limited"], lat["max_multiplets"], lat["max_modeled_k_let"]) == (limited, mm, mmk)
            prior = R.log_prior(states, est, ng, limited, mmk, mk)
            fin = np.isfinite(prior)
            assert np.array_equal(fin, np.isfinite(lat["prior"])) and np.all(np.isneginf(lat["prior"][~fin]))
            assert np.all(np.abs(lat["prior"][fin] - prior[fin]) <= 1e-13), (n, k, ng, mk)
    assert len(E.jibes_latent_states(130, 16, 300)["states"]) == 970
    assert int(np.isneginf(E.jibes_latent_states(400, 3, 2000)["prior"]).sum()) == 11      # the quirk
    fr = np.array([0.5, 0.3, 0.2])
    st, lim, _, mmk, est = R.latent_state_setup(400, 3, 2000)
    want = R.log_prior(st, est, 2000, lim, mmk, blank=0.1, freqs=fr)
    got = E.jibes_latent_states(400, 3, 2000, estimated_cells=est, blank_prob=0.1, freqs=fr)["prior"]
    fin = np.isfinite(want)
    assert np.all(np.abs(got[fin] - want[fin]) <= 1e-13) and np.array_equal(fin, np.isfinite(got))
    for k, mk in ((17, 3), (3, 4)):
        with pytest.raises(E.CrgpuError) as ei:
            E.jibes_latent_states(100, k, 2000, mk)
        assert ei.value.code == ERANGE
    with pytest.raises(E.CellEstimateCantConverge):
        E.jibes_expected_cells(70000, 95000)
    assert E.jibes_expected_cells(0, 2000) == 0.0
    assert E.G19_N_GEMS == R.G19_N_GEMS == {"MT": 95000, "LT": 9500, "HT": 190000}


def test_expected_cells_against_the_recorded_reference():
    from cellranger_amd import engine as E

    g = golden()
    for (n, ng), want in zip(g["ec_cases"], g["ec_expect"]):
        assert abs(E.jibes_expected_cells(int(n), int(ng)) - want) <= 1e-5      # BFGS stops within 2.4e-6 cells of the root (recorded)


def test_initial_parameters_equal_the_reference():
    from cellranger_amd import engine as E

    g = golden()
    for ci in range(int(g["init_n_cases"])):
        p = "init%d_" % ci
        bg, fg, sd = E.jibes_initial_parameters(g[p + "Y"], g[p + "calls"])
        assert bg.tobytes() == g[p + "bg"].tobytes() and fg.tobytes() == g[p + "fg"].tobytes(), ci
        assert np.all(np.abs(sd.view(np.int64) - g[p + "sd"].view(np.int64)) <= 2), ci
    rng = np.random.RandomState(8)
    for n, k in ((300, 12), (1000, 5), (9, 2)):      # sums long enough for numpy's pairwise blocks
        Y, calls = rng.uniform(0, 4, (n, k)), rng.randint(-1, k, n)
        bg, fg, sd = E.jibes_initial_parameters(Y, calls)
        rb, rf, rs = R.initial_parameters(Y, calls)
        assert bg.tobytes() == rb.tobytes() and fg.tobytes() == rf.tobytes() and np.all(np.abs(sd.view(np.int64) - rs.view(np.int64)) <= 2)
