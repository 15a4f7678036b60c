"""GPU parity of the count stage on constructed boundary cases (tests/count_cases.py), bit for bit against the oracle run per
(barcode, library): segments of exactly UC_SMALL, UES_CAP, UE_CAP keys and one more, in a tile, on its end and across tile
multiples; owners across headless tiles; winners past the halo of the giant chunks; full buckets; the rules of correct_umis;
libraries without correction; low-support groups over LF_TILE boundaries and groups whose sort hashes collide.  Every case
asserts its own structure (count_cases.check_claims) before any result is compared, so a case that no longer hits its edge
fails instead of passing."""
import numpy as np
import pytest

import count_cases as CC

pytestmark = pytest.mark.gpu

STAT_DISTINCT_KEYS = 9              # CRGPU_STAT_DISTINCT_KEYS
STAT_LOW_SUPPORT_CANDIDATES = 10    # CRGPU_STAT_LOW_SUPPORT_CANDIDATES


def _run(case):
    """build_keys + count_keys (molecules, triplets, the two counters) and count_records (per-read DupInfo) on a context of
    the case's own: whitelist-rank keys, the synthetic list"""
    import gpu_helpers as G

    c = G.fresh_ctx(dense=False)
    wl = case.whitelist()
    for lib in range(case.n_libs):
        c.set_whitelist(lib, wl, length=16)
    _, canon_sorted = c.canon_order()
    assert np.array_equal(canon_sorted, wl)          # a barcode's rank is its value
    c.set_key_layout(case.n_features, case.umi_len, case.n_libs, case.mux_mask)
    if case.umi_min_len is not None:
        c.set_umi_min_len(case.umi_min_len)
    r = case.records
    n = len(r["idx"])
    d_idx, d_umi, d_uq = c.upload(r["idx"]), c.upload(r["umi"]), c.upload(r["umi_qualn"])
    d_ft, d_fl_in = c.upload(r["feature"]), c.upload(r["flags"])
    d_len = c.upload(r["ulen"]) if case.umi_min_len is not None else None
    recs = c.records(n, case.umi_len, d_idx, d_umi, d_uq, d_ft, d_fl_in, d_umi_len=d_len)
    keys = c.empty(n, np.uint64)
    nk = c.build_keys(recs, keys)
    assert nk == n                                    # every read of a case is valid
    cnt = c.count_keys(keys, nk)
    out = dict(nd=c.stat(STAT_DISTINCT_KEYS), n_cand=c.stat(STAT_LOW_SUPPORT_CANDIDATES), mol=cnt.molecules(), triplets=cnt.triplets())
    cnt.free()
    d_pu, d_rc, d_fl = c.empty(n, np.uint32), c.empty(n, np.uint32), c.empty(n, np.uint8)
    cnt3 = c.count_records(recs, d_pu, d_rc, d_fl)
    out.update(processed_umi=d_pu.to_host(count=n), read_count=d_rc.to_host(count=n), flags=d_fl.to_host(count=n))
    out["nd_records"], out["n_cand_records"] = c.stat(STAT_DISTINCT_KEYS), c.stat(STAT_LOW_SUPPORT_CANDIDATES)
    mol3 = cnt3.molecules()
    for k, v in out["mol"].items():
        assert np.array_equal(mol3[k], v), "count_records and count_keys: molecule %s" % k
    for a, b in zip(cnt3.triplets(), out["triplets"]):
        assert np.array_equal(a, b)
    cnt3.free()
    c.close()
    return out


def _check(case):
    from test_count_cases_host import assert_same_results, oracle_expected

    d = CC.check_claims(case)                         # the structure first
    got = _run(case)
    # path evidence: the distinct keys are the builder's, and the candidate filter has no false negatives
    assert got["nd"] == got["nd_records"] == d.nd == case.nd
    assert got["n_cand"] >= d.n_group_keys and got["n_cand_records"] >= d.n_group_keys
    exp = oracle_expected(case)
    assert_same_results(got, exp, case.name)
    if case.mux_mask:   # UmiCorrection::Disable: nothing of those libraries moves, low support still applies
        off = ((case.mux_mask >> (case.records["flags"] & 0x0F)) & 1) != 0
        assert off.any() and not (got["flags"][off] & 2).any() and (got["flags"][off] & 4).any()
        assert np.array_equal(got["processed_umi"][off], case.records["umi"][off])
    return d, got, exp


@pytest.mark.parametrize("name", list(CC.SMALL_CASES))
def test_constructed_case_equals_the_oracle(name):
    """The size classes of UMI correction at both sides of UC_SMALL, UES_CAP and UE_CAP, at offsets 0, 1, UC_TILE - 1 and on
    the tile end; headless tiles; abutting segments; full buckets; the rules; other UMI lengths (3, 11, 16, mixed per read);
    a library without correction; the low-support groups and their LF_TILE placements."""
    d, got, exp = _check(CC.get_case(name))
    if name == "small_L12":
        assert ((got["flags"] & 2) != 0).sum() > 1000 and ((got["flags"] & 4) != 0).sum() > 100


def test_giant_segment_winners_past_the_halo_and_in_other_chunks():
    """One segment of 2 UE_CAP + 5 keys: winners that lie more than GI_HALO behind the staged window along the run of equal
    high halves (the walk goes on in device memory), winners in another chunk's low-half table (k_giant_probe + atomicMax),
    a low-half column over several full buckets.  check_claims asserts each of those positions."""
    case = CC.get_case("giant")
    assert sum(1 for c in case.claims if c["kind"] == "far" and c["same_high_half"]) == 2
    assert sum(1 for c in case.claims if c["kind"] == "far" and not c["same_high_half"]) == 2
    d, got, exp = _check(case)
    # the far winners took their reads: each far key's reads carry the winner's UMI
    r = case.records
    for c in case.claims:
        if c["kind"] == "far":
            reads = (r["idx"] == c["key"][0]) & (r["umi"] == c["key"][4])
            assert reads.any() and (got["processed_umi"][reads] == c["winner"][4]).all() and ((got["flags"][reads] & 2) != 0).all()


def test_groups_with_colliding_sort_hashes_stay_apart():
    """250 000 distinct 64-bit keys (vbits = 18).  Pairs of different (barcode, UMI) groups whose 32-bit sort keys agree: in
    the first kind the extra hash bits of the payload differ, in the second they agree too and only the exact group_id
    comparison tells the groups apart.  One group of a pair has a shared maximum (all low), the other a strict winner; merged,
    the winner would be low as well."""
    case = CC.get_case("collisions")
    d = CC.describe(case)
    n = CC.check_collisions(case, d)
    assert n[1] >= 1 and n[2] >= 1
    d, got, exp = _check(case)
    r = case.records
    (claim,) = [c for c in case.claims if c["kind"] == "collision"]
    for g1, g2, kind in claim["pairs"]:
        m1 = (r["idx"] == g1 >> 24) & (r["umi"] == g1 & 0xFFFFFF)
        m2 = (r["idx"] == g2 >> 24) & (r["umi"] == g2 & 0xFFFFFF)
        assert ((got["flags"][m1] & 4) != 0).all()                                  # shared maximum: every read low
        win = m2 & (r["feature"] == 0)
        assert not (got["flags"][win] & 4).any() and ((got["flags"][m2 & ~win] & 4) != 0).all()


@pytest.mark.parametrize("S", CC.TRANSLATED)
def test_segment_results_do_not_depend_on_the_offset(S):
    """The same segment at offsets 0, 1, UC_TILE - UC_SMALL - 1 and UC_TILE - 1 (in a tile, across one or more multiples,
    other chunk and tile positions): its molecules and the DupInfo of its reads are identical.  No oracle involved."""
    ref = None
    for off in CC.TRANSLATED_OFFSETS:
        case = CC.translation_case(S, off)
        d = CC.check_claims(case)
        got = _run(case)
        assert got["nd"] == d.nd
        reads = case.records["idx"] == case.segment_bc
        mol = got["mol"]["bc"] == case.segment_bc
        seg = [got[k][reads] for k in ("flags", "processed_umi", "read_count")] + [got["mol"][k][mol] for k in ("lib", "feature", "umi", "read_count", "utype")]
        assert len(seg[0]) > S and len(seg[3]) > 0
        if ref is not None:
            for a, b in zip(seg, ref):
                assert np.array_equal(a, b), "S = %d at offset %d" % (S, off)
        ref = seg


@pytest.mark.parametrize("overlap", [None, "0", "2"])
def test_composite_case_on_one_and_two_streams(overlap, monkeypatch):
    """the composite case with the low-support search beside UMI correction (CRGPU_DEDUP_OVERLAP=2), behind it (=0) and as by
    default: the oracle's results every time, hence identical ones"""
    if overlap is None:
        monkeypatch.delenv("CRGPU_DEDUP_OVERLAP", raising=False)
    else:
        monkeypatch.setenv("CRGPU_DEDUP_OVERLAP", overlap)
    _check(CC.get_case("small_L12"))
