"""CPU-side checks of the multiplexed-Flex entry points (no GPU): the symbols are declared, exported and bound, they refuse a NULL
context, the three structs have one layout in the header, the library (crgpu_abi_layout), the ctypes table, the Rust block of
INTEGRATION.md and include/crgpu.hpp, and every host function (overlap rows, Antibody thresholds, suspicious pairings, occupancy
summary, the threshold simulation of the engine) equals the restatement tests/rtl_tags_numpy.py on the hand cases of
tests/test_rtl_tags_restatement.py and on 200 seeded random inputs.  f64 values are compared as bit patterns, NaN equal to NaN."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import rtl_tags_numpy as R
import test_abi_and_host as A
import test_rtl_tags_restatement as H

ROOT = A.ROOT
NEW_SYMBOLS = ["crgpu_rtl_tags_dev", "crgpu_rtl_sample_columns_dev", "crgpu_rtl_gem_runs_dev", "crgpu_rtl_medians_dev",
               "crgpu_rtl_overlap_rows", "crgpu_rtl_ab_thresholds", "crgpu_rtl_suspicious_pairings", "crgpu_rtl_occupancy_summary",
               "crgpu_rtl_remove_high_occupancy_dev"]
EINVAL, ERANGE = -1, -6
STRUCTS = {"crgpu_rtl_gem_runs": ("RtlGemRuns", "CrgpuRtlGemRuns", 40040), "crgpu_rtl_overlap_row": ("RtlOverlapRow", "CrgpuRtlOverlapRow", 40),
           "crgpu_rtl_high_occupancy": ("RtlHighOccupancy", "CrgpuRtlHighOccupancy", 64)}


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


def test_new_entry_points_refuse_a_null_context_and_bad_arguments():
    from cellranger_amd import _lib

    L = _lib.load()
    m, runs, occ, out = _lib.MatrixDevView(), _lib.RtlGemRuns(), _lib.RtlHighOccupancy(), C.c_void_p()
    a8, a64 = np.zeros(4, np.uint8), np.zeros(4, np.uint64)
    assert L.crgpu_rtl_tags_dev(None, C.byref(m), _lib.ptr(a8), 1, None, 0, 0, None, _lib.ptr(a64), None) == EINVAL
    assert L.crgpu_rtl_sample_columns_dev(None, None, 0, _lib.ptr(a8), 1, 1, 0, None, 0, C.byref(out), _lib.ptr(a64)) == EINVAL
    assert L.crgpu_rtl_gem_runs_dev(None, C.byref(m), None, 1, None, 0, None, None, None, C.byref(runs)) == EINVAL
    assert L.crgpu_rtl_medians_dev(None, C.byref(m), None, None, 0, _lib.ptr(a64), _lib.ptr(a64)) == EINVAL
    assert L.crgpu_rtl_remove_high_occupancy_dev(None, C.byref(m), None, 0, 1, C.byref(out), C.byref(occ)) == EINVAL
    # the host functions need no context; they refuse missing arrays and sizes outside the limits
    n, rows = C.c_uint32(), (_lib.RtlOverlapRow * 4)()
    full = np.zeros((64, 64), np.uint64)
    assert L.crgpu_rtl_overlap_rows(None, _lib.ptr(full), _lib.ptr(a8), 2, rows, 4, C.byref(n)) == EINVAL
    assert L.crgpu_rtl_overlap_rows(_lib.ptr(a64), _lib.ptr(full), _lib.ptr(a8), 65, rows, 4, C.byref(n)) == EINVAL
    pres = np.ones(4, np.uint8)
    assert L.crgpu_rtl_overlap_rows(_lib.ptr(a64), _lib.ptr(full), _lib.ptr(pres), 4, rows, 4, C.byref(n)) == ERANGE and n.value == 6
    assert L.crgpu_rtl_overlap_rows(_lib.ptr(a64), _lib.ptr(full), _lib.ptr(pres), 4, None, 0, C.byref(n)) == 0 and n.value == 6   # size query
    assert L.crgpu_rtl_ab_thresholds(None, _lib.ptr(a64), _lib.ptr(a8), 4, _lib.ptr(a8), 4, _lib.ptr(a64)) == EINVAL
    assert L.crgpu_rtl_suspicious_pairings(rows, 1, None, None, 4, rows, C.byref(n)) == EINVAL
    z, lam, pr = C.c_uint64(), C.c_double(), C.c_uint32()
    assert L.crgpu_rtl_occupancy_summary(None, 4, 0, _lib.ptr(a64), 10, 0.5, C.byref(z), C.byref(lam), C.byref(pr)) == EINVAL
    hist = np.zeros(5, np.uint64)
    assert L.crgpu_rtl_occupancy_summary(_lib.ptr(hist), 4, 0, _lib.ptr(a64), 0, 0.5, C.byref(z), C.byref(lam), C.byref(pr)) == EINVAL   # 0 / 0
    assert (_lib.RTL_MAX_TAGS, _lib.RTL_MAX_PROBES, _lib.RTL_MAX_TYPES) == (64, 256, 8)


# ---- the structs: header == library == ctypes == Rust == C++ ---------------------------------------------------------------------
def _header_struct(name):
    with open(os.path.join(ROOT, "include", "crgpu.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    m = re.search(r"\bstruct\s+%s\s*\{(.*?)\}\s*;" % name, text, flags=re.S)
    assert m and re.search(r"typedef\s+struct\s+%s\s+%s\s*;" % (name, name), text)
    fields = []
    for decl in m.group(1).split(";"):
        decl = " ".join(decl.split())
        if not decl:
            continue
        ctype, names = decl.split(" ", 1)
        for nm in names.split(","):
            nm = nm.strip()
            arr = re.match(r"(\w+)\[(\d+)\]$", nm)
            size = A._C_SIZES[ctype]
            fields.append((arr.group(1) if arr else nm, size, size, int(arr.group(2)) if arr else 1))
    return A._layout(fields)


def _rust_struct(name, rust_name):
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        text = f.read()
    m = re.search(r"//\s*mirrors %s\b[^\n]*\n#\[repr\(C\)\]\s*pub struct %s\s*\{(.*?)\n\}" % (name, rust_name), text, flags=re.S)
    assert m, "INTEGRATION.md has no %s block" % rust_name
    body = re.sub(r"//[^\n]*", "", m.group(1))
    fields = []
    for nm, ty in re.findall(r"pub\s+(\w+)\s*:\s*(\[[^\]]+\]|[^,]+?)\s*(?:,|$)", body.replace("\n", " ")):
        arr = re.match(r"\[(\w+);\s*(\d+)\]$", ty.strip())
        base = arr.group(1) if arr else ty.strip()
        fields.append((nm, A._RUST_SIZES[base], A._RUST_SIZES[base], int(arr.group(2)) if arr else 1))
    return A._layout(fields)


@pytest.mark.parametrize("name", sorted(STRUCTS))
def test_struct_layout_agrees_everywhere(name):
    from cellranger_amd import _lib

    cls_name, rust_name, expect = STRUCTS[name]
    size, align, fields = _header_struct(name)
    assert (size, align) == (expect, 8)
    lsize, lalign, lfields = A.library_layout(name)
    assert (size, align) == (lsize, lalign)
    assert [(o, s) for _, o, s in fields] == lfields
    cls = getattr(_lib, cls_name)
    assert C.sizeof(cls) == size
    assert [(f[0], getattr(cls, f[0]).offset, getattr(cls, f[0]).size) for f in cls._fields_] == fields
    assert _rust_struct(name, rust_name) == (size, align, fields)
    with open(os.path.join(ROOT, "include", "crgpu.hpp")) as f:
        hpp = f.read()
    assert re.search(r"static_assert\(sizeof\(%s\) == %d\b" % (name, size), hpp)      # crgpu.hpp uses the C struct itself
    with open(os.path.join(ROOT, "include", "crgpu.h")) as f:
        hdr = f.read()
    for macro, v in (("MAX_TAGS", 64), ("MAX_PROBES", 256), ("MAX_TYPES", 8), ("KIND_RTL", 0), ("KIND_ANTIBODY", 1), ("KIND_OTHER", 2)):
        assert int(re.search(r"#define CRGPU_RTL_%s (\d+)" % macro, hdr).group(1)) == v == getattr(_lib, "RTL_" + macro)


# ---- host functions == restatement -----------------------------------------------------------------------------------------------
def _bits(x):
    return np.asarray(x, np.float64).view(np.uint64)


def _tables(groups, ids):
    """what the device reports for a map id -> {gel: n}: gems per tag, the pair table, the keys"""
    T = len(ids)
    gems, common, present = np.zeros(T, np.uint64), np.zeros((T, T), np.uint64), np.zeros(T, np.uint8)
    for t, i in enumerate(ids):
        if i in groups:
            present[t] = 1
            gems[t] = len(groups[i])
    for a in range(T):
        for b in range(a + 1, T):
            if ids[a] in groups and ids[b] in groups:
                common[a, b] = len(set(groups[ids[a]]) & set(groups[ids[b]]))
    return gems, common, present


def _same_rows(got, ids, ref):
    assert len(got) == len(ref)
    for g, r in zip(got, ref):
        assert (ids[g["tag1"]], ids[g["tag2"]], g["gems1"], g["gems2"], g["common_gems"]) == r[:5]
        assert _bits(g["overlap"]) == _bits(r[5]) or (np.isnan(g["overlap"]) and np.isnan(r[5]))


POOL = ["AB001", "AB002", "BC001", "BC002", "BC003", "BC025", "CR001", "XYZ"]      # ascending


def _random_groups(rng):
    ids = [i for i in POOL if rng.rand() < 0.8] or ["BC001"]
    groups = {}
    for i in ids:
        if rng.rand() < 0.85:
            gels = rng.choice(12, rng.randint(0, 9), replace=False)
            groups[i] = {int(g): int(rng.randint(1, 5)) for g in gels}
    return ids, groups


def _kinds(ids):
    from cellranger_amd import engine as E

    k = np.array([E.rtl_tag_kind(i) for i in ids], np.uint8)
    assert [("RTL", "Antibody").index(R.categorize(i)) if R.categorize(i) in ("RTL", "Antibody") else 2 for i in ids] == k.tolist()
    return k


def test_overlap_rows_and_pairings_of_the_hand_cases():
    from cellranger_amd import engine as E

    groups = R.group(H.W5, H.IDS3)
    rows = E.rtl_overlap_rows(*_tables(groups, H.IDS3))
    _same_rows(rows, H.IDS3, R.overlap_rows(groups))
    assert [r["overlap"] for r in rows] == [2 / 3, 0.5, 1.0]
    nan = E.rtl_overlap_rows(*_tables({"AB001": {}, "BC001": {3: 1}}, ["AB001", "BC001"]))
    assert len(nan) == 1 and np.isnan(nan[0]["overlap"]) and nan[0]["gems1"] == 0
    ids = ["AB001", "AB002", "BC001", "BC002"]
    combined = {"AB001": {0: 40, 1: 3, 2: 20}, "AB002": {0: 100, 1: 10}, "BC001": {0: 1, 2: 1}, "BC002": {0: 1}}
    all_rows = E.rtl_overlap_rows(*_tables(combined, ids))
    got = E.rtl_suspicious_pairings(all_rows, _kinds(ids), [-1, -1, 0, 1])
    _same_rows(got, ids, [("BC001", "AB002", 2, 2, 1, 0.5), ("BC002", "AB001", 1, 3, 1, 1.0)])
    got = E.rtl_suspicious_pairings(all_rows, _kinds(ids), [-1, -1, 0, -1])      # one configured pairing
    _same_rows(got, ids, R.filter_suspicious(R.overlap_rows(combined), {"BC001": "AB001"}))
    assert [(ids[g["tag1"]], ids[g["tag2"]]) for g in got] == [("BC001", "AB002"), ("BC002", "AB001"), ("BC002", "AB002")]


def test_ab_thresholds_of_the_hand_cases():
    from cellranger_amd import _lib
    from cellranger_amd import engine as E

    kind = [1, 1, 0, 0]      # AB001, AB002, BC001, BC002
    none = np.uint64(0xFFFFFFFFFFFFFFFF)
    assert E.rtl_ab_thresholds([30, 100], [2, 1], [0, 1], kind).tolist() == [3, 10, none, none]
    assert E.rtl_ab_thresholds([30, 100], [0, 1], [0, 1], kind).tolist() == [none, 10, none, none]        # removed: no cell with counts
    assert E.rtl_ab_thresholds([4, 5, 15, 25], [1, 1, 1, 1], [0, 1, 2, 3], [1, 1, 1, 1]).tolist() == [0, 1, 2, 3]
    for bad in (([30, 100], [2, 1], [0, 2], kind),            # a median under an RTL identifier: the reference's assert_eq
                ([30, 100], [2, 1], [0, 0], kind),            # two probe ranks with medians on one tag
                ([30, 100], [2, 1], [0, 0xFF], kind)):        # a median and no tag
        with pytest.raises(_lib.CrgpuError) as e:
            E.rtl_ab_thresholds(*bad)
        assert e.value.code == EINVAL


def test_occupancy_summary_and_threshold_of_the_hand_case():
    from cellranger_amd import engine as E

    hist, cpp = [0, 2, 2, 1], [4, 3, 2]
    got = E.rtl_occupancy_summary(hist, 5, cpp, 10, 0.5)
    assert got == dict(histogram={1: 2, 2: 2, 3: 1, 0: 0}, estimated_lambda=9 / 5, total_probe_barcodes=3)
    got = E.rtl_occupancy_summary(hist, 5, cpp)
    assert got["histogram"][0] == 69691 and got["estimated_lambda"] == 9 / 69696
    assert E.rtl_occupancy_summary(hist, 5, cpp, 4, 1.0)["histogram"][0] == 0
    probes = [p for _, p in H.W5]
    first = [0, 1, 4]      # the first cell column of every probe rank in W5
    assert E.high_occupancy_gem_threshold(1.8, cpp, first, 5000) == R.threshold(1.8, probes, 5000) == 3
    assert E.high_occupancy_gem_threshold(0.0, cpp, first) == 0


@pytest.mark.parametrize("block", range(4))
def test_host_functions_equal_the_restatement_on_random_inputs(block):
    from cellranger_amd import engine as E

    for seed in range(block * 50, block * 50 + 50):      # 200 in all
        rng = np.random.RandomState(seed)
        ids, groups = _random_groups(rng)
        rows = E.rtl_overlap_rows(*_tables(groups, ids))
        _same_rows(rows, ids, R.overlap_rows(groups))
        # a random pairing of the RTL identifiers with antibody identifiers
        rtl = [i for i in ids if R.categorize(i) == "RTL"]
        ab = [i for i in ids if R.categorize(i) == "Antibody"]
        pairings = {r: ab[rng.randint(len(ab))] for r in rtl if ab and rng.rand() < 0.5}
        pw = np.full(len(ids), -1, np.int32)
        for r, a in pairings.items():
            pw[ids.index(r)] = ids.index(a)
        _same_rows(E.rtl_suspicious_pairings(rows, _kinds(ids), pw), ids, R.filter_suspicious(R.overlap_rows(groups), pairings))
        # thresholds
        n_probe = rng.randint(1, 17)
        med = rng.randint(0, 4000, n_probe)
        nz = rng.randint(0, 3, n_probe)
        low = E.rtl_ab_thresholds(med, nz, np.arange(n_probe), np.ones(n_probe, np.uint8))
        assert low.tolist() == [int(R.rust_round(0.1 * float(m))) if k else 0xFFFFFFFFFFFFFFFF for m, k in zip(med, nz)]
        # occupancy
        n_probe = rng.randint(1, 9)
        cells = sorted(set((int(g), int(p)) for g, p in zip(rng.randint(0, 40, 60), rng.randint(0, n_probe, 60))))
        parts, rec = int(rng.randint(0, 200)), [1 / 1.65, 0.5, 0.37][seed % 3]
        hist, lam, probes, per_gem = R.occupancy(cells, parts, rec)
        h = np.zeros(n_probe + 1, np.uint64)
        for k, n in hist.items():
            if k:
                h[k] = n
        cpp, first = np.zeros(n_probe, np.uint64), np.full(n_probe, 0xFFFFFFFFFFFFFFFF, np.uint64)
        for c, (_, p) in enumerate(cells):
            cpp[p] += 1
            first[p] = min(int(first[p]), c)
        got = E.rtl_occupancy_summary(h, len(per_gem), cpp, parts, rec)
        assert got["histogram"] == {k: n for k, n in hist.items() if n or k == 0} and got["total_probe_barcodes"] == probes
        assert _bits(got["estimated_lambda"]) == _bits(lam)
        # the threshold simulation: real numpy on both sides, the probabilities in order of first appearance.  lambda of a loaded well
        lam_sim = [0.05, 0.4, 1.3, 2.5][seed % 4]
        order = [p for _, p in sorted(cells, key=lambda gp: (gp[1] % 3, gp))]       # any order of the cells: the first columns follow it
        cpp2, first2 = np.zeros(n_probe, np.uint64), np.full(n_probe, 0xFFFFFFFFFFFFFFFF, np.uint64)
        for c, p in enumerate(order):
            cpp2[p] += 1
            first2[p] = min(int(first2[p]), c)
        assert E.high_occupancy_gem_threshold(lam_sim, cpp2, first2, 2000) == R.threshold(lam_sim, order, 2000)
