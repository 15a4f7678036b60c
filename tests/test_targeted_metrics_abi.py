"""CPU-side checks of the targeted-metrics entry points (no GPU): the symbols are declared, exported and bound, they refuse a NULL
context and bad arguments, the three structs have one layout in the header, the library (crgpu_abi_layout), the ctypes table, the
Rust block of INTEGRATION.md and include/crgpu.hpp, and the host function crgpu_targeted_rpu_stats equals the restatement
tests/targeted_metrics_numpy.py (pandas, literally the reference's calls) on the hand cases and on 200 seeded random tallies.

Median, percentile and iqr / median are compared bit for bit, NaN equal to NaN: they are numpy's linear rule between two order
statistics.  So are the saturation, the gene counts and the list of quantifiable features.  Mean and cv are held within
R.float_bounds, which derives its bounds from the two summation schemes (see there); nothing is fitted to what is observed (observed
here: at most 2 ulp).  The log10 column: the C library's log10 and numpy's each claim less than 1 ulp, so the library's own
q_value_out is held within 2 ulp of numpy's; the Python layer (engine.targeted_rpu_stats) returns numpy's values, bit for bit."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import targeted_metrics_numpy as R
import test_abi_and_host as A
import test_rtl_tags_abi as T
import test_subsample_abi as SA

ROOT = A.ROOT
NEW_SYMBOLS = ["crgpu_feature_metrics_dev", "crgpu_targeted_rpu_stats", "crgpu_rpu_gmm_dev"]
EINVAL = -1
STRUCTS = {"crgpu_rpu_stats": ("RpuStats", "CrgpuRpuStats", 256, T), "crgpu_rpu_gmm_args": ("RpuGmmArgs", "CrgpuRpuGmmArgs", 32, SA),
           "crgpu_rpu_gmm_result": ("RpuGmmResult", "CrgpuRpuGmmResult", 120, T)}
GOLDEN = os.path.join(ROOT, "tests", "golden", "targeted_metrics_reference.npz")
TALLY_KEYS = ("num_umis", "num_reads", "num_umis_cells", "num_reads_cells")


@pytest.fixture(scope="module", autouse=True)
def built_library():
    from cellranger_amd import build

    build.build()


def test_new_symbols_are_declared_exported_and_bound():
    from cellranger_amd import _lib

    declared = A.header_symbols()
    L = C.CDLL(_lib.LIB_PATH)
    for s in NEW_SYMBOLS:
        assert s in declared, s
        assert hasattr(L, s), s
        assert s in _lib.SYMBOLS, s
    assert _lib.load().crgpu_abi_version() == 3      # additive: no bump
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        text = f.read()
    for s in NEW_SYMBOLS:
        assert re.search(r"pub fn %s\(" % s, text), s
    with open(os.path.join(ROOT, "include", "crgpu.h")) as f:
        hdr = f.read()
    assert int(re.search(r"#define CRGPU_GMM_STARTS (\d+)", hdr).group(1)) == _lib.GMM_STARTS == R.N_STARTS == 5152
    assert int(re.search(r"#define CRGPU_TARGETED_MIN_UMIS (\d+)", hdr).group(1)) == _lib.TARGETED_MIN_UMIS == R.MIN_UMIS == 10


def test_new_entry_points_refuse_null_and_bad_arguments():
    from cellranger_amd import _lib

    L = _lib.load()
    st, res, args = _lib.RpuStats(), _lib.RpuGmmResult(), _lib.RpuGmmArgs()
    a = np.ones(3, np.uint64)
    flags = np.ones(3, np.uint8)
    v = np.zeros(3)
    assert L.crgpu_feature_metrics_dev(None, None, 3, 1, None, 0, _lib.ptr(a), None, None, None) == EINVAL
    assert L.crgpu_rpu_gmm_dev(None, _lib.ptr(v), _lib.ptr(flags), 3, C.byref(args), C.byref(res)) == EINVAL
    p = _lib.ptr
    assert L.crgpu_targeted_rpu_stats(3, p(a), p(a), p(a), p(a), p(flags), None, None, None, None, None) == EINVAL
    assert L.crgpu_targeted_rpu_stats(3, None, p(a), p(a), p(a), p(flags), None, C.byref(st), None, None, None) == EINVAL
    assert L.crgpu_targeted_rpu_stats(3, p(a), p(a), p(a), p(a), None, None, C.byref(st), None, None, None) == EINVAL
    assert b"NULL" in L.crgpu_last_error(None)
    assert L.crgpu_targeted_rpu_stats(0, None, None, None, None, None, None, C.byref(st), None, None, None) == 0      # no feature: no error
    assert st.n_quantifiable_total == 0 and st.mean[0] == 0.0 and math.isnan(st.pcr_dupe_reads_frac_on_target)
    assert L.crgpu_targeted_rpu_stats(3, p(a), p(a), p(a), p(a), p(flags), None, C.byref(st), None, None, None) == 0  # every output list may be NULL


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
    assert re.search(r"static_assert\(sizeof\(%s\) == %d\b" % (name, size), hpp)      # crgpu.hpp uses the C struct itself


# ---- crgpu_targeted_rpu_stats == restatement ------------------------------------------------------------------------------------------
def _bits(x):
    return np.asarray(x, np.float64).view(np.uint64)


def _ulps(a, b):
    return np.abs(np.asarray(a, np.float64).view(np.int64) - np.asarray(b, np.float64).view(np.int64))


def _raw_q_values(tallies, is_targeted, is_gex):
    """q_value_out of the library itself (the Python layer replaces it by numpy's log10)"""
    from cellranger_amd import _lib

    a = [np.ascontiguousarray(x, dtype=np.uint64) for x in tallies]
    F = len(a[0])
    tg = np.ascontiguousarray(is_targeted, dtype=np.uint8)
    gx = None if is_gex is None else np.ascontiguousarray(is_gex, dtype=np.uint8)
    st, qv = _lib.RpuStats(), np.zeros(F)
    p = _lib.ptr
    assert _lib.load().crgpu_targeted_rpu_stats(F, p(a[0]), p(a[1]), p(a[2]), p(a[3]), p(tg), p(gx), C.byref(st), None, p(qv), None) == 0
    return qv[:int(st.n_quantifiable_total)]


def _same_stats(tallies, is_targeted, is_gex):
    from cellranger_amd import engine as E

    got = E.targeted_rpu_stats(*tallies, is_targeted, is_gex)
    ref, pfm = R.rpu_stats(*tallies, is_targeted, is_gex)
    assert sorted(got) == sorted(ref)
    fb = R.float_bounds(pfm)
    worst = 0
    for k, v in ref.items():
        if k.startswith("q_"):
            assert got[k].dtype == v.dtype and got[k].tobytes() == v.tobytes(), k
            continue
        a, v = float(got[k]), float(v)
        if math.isnan(a) and math.isnan(v):
            continue
        if k in fb:
            if a != v:
                print(k, a, v, "ulps", int(_ulps(a, v)), "bound (rel, abs) in 2^-52", fb[k])
            worst = max(worst, int(_ulps(a, v)))
            assert abs(a - v) <= (fb[k][0] * abs(v) + fb[k][1]) * 2.0 ** -52, (k, a, v, fb[k])
        else:
            assert _bits(a) == _bits(v), (k, a, v)
    raw = _raw_q_values(tallies, is_targeted, is_gex)
    assert len(raw) == len(ref["q_value"]) and (len(raw) == 0 or _ulps(raw, ref["q_value"]).max() <= 2)
    return worst


def test_stats_of_the_hand_cases():
    from cellranger_amd import engine as E

    g = dict(np.load(GOLDEN))
    names = [str(k) for k in g["stats_names"]]
    for i in range(int(g["n_stats_cases"])):
        c = {k: g["stats%d_%s" % (i, k)] for k in TALLY_KEYS + ("is_targeted", "is_gex")}
        _same_stats([c[k] for k in TALLY_KEYS], c["is_targeted"], c["is_gex"])
        got = E.targeted_rpu_stats(**c)
        for k, v in zip(names, g["stats%d_expect" % i]):      # the recorded pandas calls; these small cases are exact throughout
            assert (math.isnan(got[k]) and math.isnan(v)) or abs(got[k] - v) <= 4 * 2.0 ** -52 * abs(v), (i, k, got[k], v)
    # hand-computed: three on-target quotients 3.1, 1.6, 10 / 3 in cells
    c = {k: g["stats0_" + k] for k in TALLY_KEYS + ("is_targeted", "is_gex")}
    got = E.targeted_rpu_stats(**c)
    assert got["median_reads_per_umi_per_gene_cells_on_target"] == 3.1 and got["perc80_reads_per_umi_per_gene_cells_on_target"] == 3.1 + (40 / 12 - 3.1) * (1.6 - 1.0)
    assert got["num_genes_not_detected_on_target"] == 1 and got["num_genes_quantifiable_on_target"] == 3 and list(got["q_feature"]) == [0, 1, 2, 5, 7]
    assert got["mean_reads_per_umi_per_gene_cells_off_target"] == (30 / 11 + 44 / 40) / 2
    # nothing quantifiable: every statistic is 0.0
    c = {k: g["stats3_" + k] for k in TALLY_KEYS + ("is_targeted", "is_gex")}
    got = E.targeted_rpu_stats(**c)
    assert all(got["%s_reads_per_umi_per_gene%s" % (n, s)] == 0.0 for n in E.RPU_STAT_NAMES for s in E.RPU_STAT_SUFFIXES) and len(got["q_value"]) == 0


@pytest.mark.parametrize("block", range(4))
def test_stats_equal_the_restatement_on_random_tallies(block):
    worst = 0
    for seed in range(block * 50, block * 50 + 50):      # 200 in all
        rng = np.random.RandomState(seed)
        F = int(rng.choice([0, 1, 2, 3, 5, 9, 40, 200, rng.randint(10, 700)]))
        uc = (rng.randint(0, 60, F) * (rng.rand(F) < 0.8)).astype(np.uint64)
        u = uc + (rng.randint(0, 30, F) * (rng.rand(F) < 0.7)).astype(np.uint64)
        if seed % 3 == 0 and F:
            u[rng.randint(0, F)] = 0      # 0 / 0 in the all-barcodes column (not a consistent tally, but the rule must hold)
        rcell = (uc * (1 + rng.rand(F) * 4)).astype(np.uint64)
        r = rcell + ((u - np.minimum(u, uc)) * (1 + rng.rand(F) * 3)).astype(np.uint64)
        r[u == 0] = 0
        if seed % 5 == 0 and F > 2:
            rcell[:] = uc * 3      # equal quotients: std 0, iqr 0
        tg = (rng.rand(F) < [0.5, 0.0, 1.0][seed % 3 if seed % 7 == 0 else 0]).astype(np.uint8)
        gx = None if seed % 4 == 0 else (rng.rand(F) < 0.9).astype(np.uint8)
        worst = max(worst, _same_stats([u, r, uc, rcell], tg, gx))
    print("largest difference of a mean or cv in this block: %d ulp" % worst)
