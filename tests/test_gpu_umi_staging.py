"""GPU parity of UMI correction where staging loads meet the ends of the array (umi_correct.h: every load of a tile is requested
from an address clamped into [0, nd - 1] and the range checks are applied to the values; the edge and giant kernels stage up
to the last key): arrays that end one key into a tile or a staging round, one key short of it and exactly on it; corrections out
of position 0 and onto position nd - 1; edge segments of every size class as the last segment of the array; giant segments at
either end of the array with winners beside the clipped halo; a library without correction.  The cases are built with the
helpers of tests/count_cases.py, assert their own structure, and are compared bit for bit with the oracle through the public
count entries (molecules, read counts, triplets, per-read DupInfo), on one stream and on two."""
import numpy as np
import pytest

import count_cases as CC

pytestmark = pytest.mark.gpu

L = 12
T, UC_SMALL, UES_CAP, UE_CAP = CC.UC_TILE, CC.UC_SMALL, CC.UES_CAP, CC.UE_CAP
ROUND = 256   # positions of one staging round of the tile kernel (its workgroup size)
BASE = CC.base_umi(L)


# ---- segments with a known move --------------------------------------------------------------------------------------------------
def _front_keys(rng, n_pad, feature=5):
    """a segment whose FIRST key (count 1) moves onto its second (count 3): the two smallest UMIs, one base apart"""
    a = BASE & ~3
    keys = [(feature, 0, L, a, 1, 0), (feature, 0, L, a | 1, 3, 1)]
    return keys + CC.far_padding(keys, n_pad, L, rng, feature=feature), a, a | 1


def _back_keys(rng, n_pad, feature=5):
    """a segment whose last key but one (count 1) moves onto its LAST (count 3): the two largest UMIs (first base T)"""
    d = (3 << (2 * (L - 1))) | (BASE & ((1 << (2 * (L - 1))) - 1))
    keys = [(feature, 0, L, d ^ 1, 1, 0), (feature, 0, L, d, 3, 0)]
    return CC.far_padding(keys, n_pad, L, rng, feature=feature) + keys, d ^ 1, d


def nd_case(nd):
    """exactly nd distinct keys: a first segment whose key 0 is corrected, single-key segments, a last segment whose target is
    key nd - 1 (its run ends at n_keys)"""
    c = CC.Case("staging_nd%d" % nd)
    rng = np.random.default_rng(nd)
    if nd == 1:
        c.add_barcode([(5, 0, L, BASE, 3, 1)], seed=1)
    elif nd == 2:
        c.add_barcode([(5, 0, L, BASE & ~3, 1, 0), (5, 0, L, (BASE & ~3) | 1, 3, 1)], seed=1)
        c.moves = [((0, 5, 0, L, BASE & ~3), (0, 5, 0, L, (BASE & ~3) | 1))]
    else:
        fk, a, b = _front_keys(rng, 2)
        bk, cc, d = _back_keys(rng, 2)
        assert nd >= len(fk) + len(bk)
        bc0, _ = c.add_barcode(fk, seed=1)
        c.filler(nd - len(fk) - len(bk))
        bc1, _ = c.add_barcode(bk, seed=2)
        c.moves = [((bc0, 5, 0, L, a), (bc0, 5, 0, L, b)), ((bc1, 5, 0, L, cc), (bc1, 5, 0, L, d))]
    assert c.nd == nd
    return c.finish()


def edge_case(S, lead):
    """a segment of S keys as the last of the array, `lead` of its keys in front of a tile multiple"""
    c = CC.Case("staging_edge_S%d_lead%d" % (S, lead))
    CC._plant_size(c, 3, 0, seed=9)                      # a head in the tile in front
    CC._plant_size(c, S, T - lead, seed=lead, ends_array=True)
    return c.finish()


def giant_end_case(at_start):
    """One segment of 2 UE_CAP + 3 keys (chunks of UE_CAP, UE_CAP and 3 keys).  at_start: it begins at key 0, so the window of
    its first chunk has no halo in front, and the key at position 3 moves onto position 0.  Otherwise it ends at key nd - 1:
    the window of the second chunk keeps 3 of its GI_HALO keys behind, the third chunk none; the last key of the second chunk
    moves onto key nd - 1, three keys into that clipped halo."""
    c = CC.Case("staging_giant_%s" % ("start" if at_start else "end"), n_wl=256)
    rng = np.random.default_rng(11 + at_start)
    keys = CC.seg_keys(2 * UE_CAP - 1, L, rng)
    lb = CC.lo_bits(L)
    hi, lo = BASE >> lb, BASE & ((1 << lb) - 1) & ~3
    top = 2 * (L - lb // 2 - 1)                           # shift of the first base inside the high half
    H = (hi & ~(3 << (top - 2))) if at_start else (hi | (3 << top))   # second base A: below every key; first base T: above
    u = [(H << lb) | lo | x for x in range(4)]
    assert all(k[3] >> lb != H for k in keys)
    counts = (9, 1, 1, 1) if at_start else (1, 1, 1, 9)
    keys += [(5, 0, L, u[x], counts[x], 0) for x in range(4)]
    if not at_start:
        c.filler(100)
    bc = c.plant("giant", keys, 0 if at_start else c.nd % T, (5, 0, L), klass="giant", chunks=3, last_chunk=3,
                 **({} if at_start else {"ends_array": True}))
    if at_start:
        c.filler(100)
        c.moves = [((bc, 5, 0, L, u[3]), (bc, 5, 0, L, u[0]))]
    else:
        c.moves = [((bc, 5, 0, L, u[0]), (bc, 5, 0, L, u[3]))]
    return c.finish()


def abut_case():
    """a segment that ends exactly on a tile multiple and one that starts there; both correct inside the tile kernel"""
    c = CC.Case("staging_abut")
    a = CC._plant_size(c, 40, T - 40, seed=1, ends_on_multiple=True)
    b = CC._plant_size(c, 40, 0, seed=2)
    c.claim(kind="abut", a=(a, 5, 0, L), b=(b, 5, 0, L))
    c.filler(10)
    return c.finish()


def mux_case():
    """library 1 without UMI correction beside library 0 with it: the same UMIs in a tile, and a segment of each across a
    tile multiple (the edge kernel skips the one of library 1 by its first key)"""
    c = CC.Case("staging_mux", n_libs=2, mux_mask=0b10)
    rng = np.random.default_rng(3)
    base = CC.seg_keys(60, L, rng, feature=5, lib=0)
    mux = [(5, 1) + k[2:] for k in base] + [(6, 1) + k[2:4] + (1 + (i % 3), 0) for i, k in enumerate(base[::2])]
    c.plant("mux-in-a-tile", base + mux, 100, (5, 1, L), klass="tile_long", mux=True)
    k2 = CC.seg_keys(70, L, rng, feature=5, lib=1)
    c.plant("mux-on-an-edge", k2 + [(6, 1) + k[2:4] + (2, 0) for k in k2[::3]], T - 30, (5, 1, L), klass="edge_small", mux=True)
    c.plant("on-an-edge", CC.seg_keys(70, L, rng, feature=5, lib=0), T - 30, (5, 0, L), klass="edge_small")
    c.filler(5)
    return c.finish()


ND_SIZES = (1, 2, ROUND - 1, ROUND, ROUND + 1, T - 1, T, T + 1, 2 * T + 1)
EDGE_SIZES = (2, UC_SMALL, UC_SMALL + 1, UES_CAP, UES_CAP + 1, UE_CAP, UE_CAP + 1)


def edge_leads(S):
    """keys of the segment in front of the tile multiple it lies across: one (the multiple at offset 1 of the segment), and
    UC_TILE - 1 (offset UC_TILE - 1) where the segment is longer than that, else all but its last key"""
    return sorted({1, min(T - 1, S - 1)})


CASES = {}
for _nd in ND_SIZES:
    CASES["nd%d" % _nd] = (lambda n=_nd: nd_case(n))
for _S in EDGE_SIZES:
    for _lead in edge_leads(_S):
        CASES["edge_S%d_lead%d" % (_S, _lead)] = (lambda s=_S, l=_lead: edge_case(s, l))
CASES["giant_start"] = lambda: giant_end_case(True)
CASES["giant_end"] = lambda: giant_end_case(False)
CASES["abut"] = abut_case
CASES["mux"] = mux_case
_built = {}


def get_case(name):
    """built once per process and never changed (the oracle's answer is cached per case name)"""
    if name not in _built:
        _built[name] = CASES[name]()
    return _built[name]


def check_structure(name, case, d, exp):
    """what the case is there for, from its records and the oracle's answer alone"""
    r = case.records
    for src, dst in getattr(case, "moves", []):
        ks, kd = CC.key_index(d, L, *src), CC.key_index(d, L, *dst)
        reads = (r["idx"] == src[0]) & (r["feature"] == src[1]) & (r["umi"] == src[4])
        assert reads.any() and (exp["processed_umi"][reads] == dst[4]).all() and ((exp["flags"][reads] & 2) != 0).all(), name
        case.move_index = getattr(case, "move_index", []) + [(ks, kd)]
    if name.startswith("nd") and d.nd >= 2:
        assert case.move_index[0][0] == 0 and case.move_index[-1][1] == d.nd - 1       # out of key 0, onto key nd - 1
        assert d.seg_start[0] == 0 and d.seg_start[-1] + d.seg_len[-1] == d.nd
    if name == "giant_start":
        assert d.seg_start[0] == 0 and d.seg_len[0] == 2 * UE_CAP + 3 and case.move_index == [(3, 0)]
    if name == "giant_end":
        s = int(d.seg_start[-1])
        assert d.seg_len[-1] == 2 * UE_CAP + 3 and s + 2 * UE_CAP + 3 == d.nd
        assert case.move_index == [(s + 2 * UE_CAP - 1, d.nd - 1)]                      # last key of chunk 1 -> key nd - 1
    if name.startswith("edge"):
        s, n = int(d.seg_start[-1]), int(d.seg_len[-1])
        assert s + n == d.nd and len(CC.multiples_inside(s, n, T)) >= 1
        assert ((exp["flags"] & 2) != 0).any() or n <= 2


@pytest.mark.parametrize("name", list(CASES))
def test_clamped_staging_equals_the_oracle(name, monkeypatch):
    from test_count_cases_host import assert_same_results, oracle_expected
    from test_gpu_count_edges import _run

    case = get_case(name)
    d = CC.check_claims(case)
    exp = oracle_expected(case)
    if not hasattr(case, "move_index"):
        check_structure(name, case, d, exp)
    for overlap in ("0", "2"):
        monkeypatch.setenv("CRGPU_DEDUP_OVERLAP", overlap)
        got = _run(case)
        assert got["nd"] == got["nd_records"] == d.nd == case.nd
        assert_same_results(got, exp, "%s, CRGPU_DEDUP_OVERLAP=%s" % (case.name, overlap))
        if case.mux_mask:   # UmiCorrection::Disable: nothing of library 1 moves
            off = ((case.mux_mask >> (case.records["flags"] & 0x0F)) & 1) != 0
            assert off.any() and not (got["flags"][off] & 2).any()
            assert np.array_equal(got["processed_umi"][off], case.records["umi"][off])
