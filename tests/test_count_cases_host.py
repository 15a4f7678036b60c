"""Host checks of the constructed count-stage cases (tests/count_cases.py): every case has the structure it claims, the
inverse of the sort hash is one, and a plain dict-based restatement of correct_umis + determine_low_support_umigenes + the
DupInfo bookkeeping (tx_annotation/src/mark_dups.rs:19-59, 87-108, 202-363) gives the oracle's answer on every small case: a
second, independent reading of the rules on exactly the inputs the device is compared on (tests/test_gpu_count_edges.py)."""
from collections import defaultdict

import numpy as np
import pytest

import count_cases as CC


# ---- the second reference --------------------------------------------------------------------------------------------------------
def py_correct(raw):
    """correct_umis (mark_dups.rs:19-59) on {(length, umi, gene): reads}: the reference's loop over the 3 L one-base
    substitutions, keeping a candidate when it has more reads than the best so far or as many and the larger UMI"""
    corr = {}
    for (L, u, g), c in raw.items():
        best_c, best_u = c, u
        for pos in range(L):
            sh = 2 * (L - 1 - pos)
            for b in range(4):
                if b == (u >> sh) & 3:
                    continue
                t = (u & ~(3 << sh)) | (b << sh)
                tc = raw.get((L, t, g), 0)
                if tc > best_c or (tc == best_c and t > best_u):
                    best_c, best_u = tc, t
        if best_u != u:
            corr[(L, u, g)] = (L, best_u, g)
    return corr


def py_mark(umi, ulen, feature, utype, qname, umi_correction):
    """BarcodeDupMarker::new + process for the reads of one (barcode, library) -> (flags, processed_umi, read_count per
    read, molecules (feature, umi, read_count, utype))"""
    n = len(umi)
    keys = [(int(ulen[i]), int(umi[i]), int(feature[i])) for i in range(n)]
    counts, min_key = defaultdict(int), {}
    for i, k in enumerate(keys):                      # DupBuilder::observe
        counts[k] += 1
        sel = (int(utype[i]), int(qname[i]))
        if k not in min_key or sel < min_key[k]:
            min_key[k] = sel
    raw = dict(counts)
    corr = py_correct(raw) if umi_correction else {}
    for k, t in corr.items():                         # one read of each corrected UMI first (:226-232)
        counts[k] -= 1
        counts[t] += 1
    by_umi = defaultdict(list)                        # determine_low_support_umigenes on those counts, zero counts included
    for k, c in counts.items():
        by_umi[k[:2]].append((k, c))
    low = set()
    for members in by_umi.values():
        mx = max(c for _, c in members)
        tied = sum(1 for _, c in members if c == mx) >= 2
        low.update(k for k, c in members if tied or c < mx)
    for k, t in corr.items():                         # the other reads (:241-246)
        counts[k] -= raw[k] - 1
        counts[t] += raw[k] - 1
    min_raw = {}                                      # the smallest raw UMI that takes a target's place (:248-268)
    for k, t in corr.items():
        if (k[1] < t[1] or t in corr) and (t not in min_raw or k[1] < min_raw[t][1]):
            min_raw[t] = k
    min_key.update({t: min_key[k] for t, k in min_raw.items()})
    flags, pu, rc = np.zeros(n, np.uint8), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    mol = [[], [], [], []]
    for i, k in enumerate(keys):                      # process (:280-363)
        ck = corr.get(k, k)
        is_low = ck in low
        is_count = not is_low and int(qname[i]) == min_key[ck][1]
        flags[i] = 1 | (2 if k in corr else 0) | (4 if is_low else 0) | (8 if is_count else 0)
        pu[i], rc[i] = ck[1], counts[ck]
        if is_count:
            for col, v in zip(mol, (ck[2], ck[1], counts[ck], int(utype[i]))):
                col.append(v)
    return flags, pu, rc, tuple(np.array(c, np.int64) for c in mol)


def oracle_mark(umi_len):
    import oracle_lib as O

    def mark(umi, ulen, feature, utype, qname, umi_correction):
        dup, uc = O.mark_dups_group(CC.ascii_umis(umi, ulen, umi_len), np.ones(len(umi), np.uint8), feature, utype=utype,
                                    qname=qname, umi_correction=umi_correction)
        flags = ((dup["has_dupinfo"] != 0) * 1 + (dup["is_corrected"] != 0) * 2 + (dup["is_low_support"] != 0) * 4 +
                 (dup["is_umi_count"] != 0) * 8 + (dup["is_filtered_target"] != 0) * 16).astype(np.uint8)
        return flags, dup["processed_umi"], dup["read_count"], (uc["feature_idx"], uc["umi"], uc["read_count"], uc["utype"])
    return mark


_expected = {}


def oracle_expected(case):
    """what the count stage has to give for a case, by the oracle per (barcode, library); computed once per case and process"""
    if case.name not in _expected:
        _expected[case.name] = CC.expected(case, oracle_mark(case.umi_len))
    return _expected[case.name]


def assert_same_results(got, exp, what=""):
    """bit for bit: every read's DupInfo (the five flag bits, processed UMI, read count), the molecule table, the triplets"""
    for bit, name in ((1, "has_dupinfo"), (2, "is_corrected"), (4, "is_low_support"), (8, "is_umi_count"), (16, "is_filtered_target")):
        assert np.array_equal((got["flags"] & bit) != 0, (exp["flags"] & bit) != 0), "%s %s" % (what, name)
    assert np.array_equal(got["flags"], exp["flags"]), what
    assert np.array_equal(got["processed_umi"], exp["processed_umi"]), "%s processed_umi" % what
    assert np.array_equal(got["read_count"], exp["read_count"]), "%s read_count" % what
    for k in ("bc", "lib", "feature", "umi", "read_count", "utype"):
        assert np.array_equal(got["mol"][k], exp["mol"][k]), "%s molecule %s" % (what, k)
    for a, b, k in zip(got["triplets"], exp["triplets"], ("barcode", "feature", "count")):
        assert np.array_equal(a, b), "%s triplet %s" % (what, k)


# ---- tests -----------------------------------------------------------------------------------------------------------------------
def test_constants_come_from_the_source():
    assert CC.UC_TILE == 256 * CC.K["UC_ITEMS"] and CC.UC_SMALL < CC.UES_CAP < CC.UE_CAP and CC.GI_HALO < CC.UE_CAP
    assert CC.K["MIX64"] == CC.K["GROUP_HASH"] and CC.K["MIX64"][1] % 2 == 1 and CC.K["MIX64"][2] % 2 == 1
    assert CC.LS_HASH_BITS == 32 and CC.LF_TILE % CC.UC_TILE == 0
    with pytest.raises(RuntimeError):
        CC._define("#define OTHER 3\n", "UC_SMALL", "nowhere")
    from cellranger_amd._lib import FLAG_NONTXOMIC

    assert CC.FLAG_NONTXOMIC == FLAG_NONTXOMIC


def test_unmix64_inverts_mix64():
    rng = np.random.default_rng(1)
    x = np.concatenate([rng.integers(0, 1 << 63, 100_000, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, 100_000, dtype=np.uint64),
                        np.array([0, 1, 2, (1 << 32) - 1, 1 << 32, 1 << 33, (1 << 33) - 1, 1 << 63, (1 << 64) - 1, CC.EMIT_XOR], np.uint64)])
    assert np.array_equal(CC.unmix64(CC.mix64(x)), x) and np.array_equal(CC.mix64(CC.unmix64(x)), x)
    assert len(np.unique(CC.mix64(x))) == len(np.unique(x))
    # the scalar recurrence, with Python's integers
    s, m1, m2 = CC.K["MIX64"]
    for v in (1, 0x0123456789ABCDEF, CC.M64):
        g = v ^ (v >> s)
        g = (g * m1) & CC.M64
        g ^= g >> s
        g = (g * m2) & CC.M64
        g ^= g >> s
        assert int(CC.mix64(np.array([v], np.uint64))[0]) == g


@pytest.mark.parametrize("name", list(CC.SMALL_CASES) + list(CC.LARGE_CASES))
def test_case_has_the_structure_it_claims(name):
    case = CC.get_case(name)
    d = CC.check_claims(case)
    assert d.nd == case.nd and len(case.claims) > 0
    r = case.records
    assert len(r["idx"]) == len(r["umi"]) == len(r["feature"]) == len(r["flags"]) == len(r["umi_qualn"]) == int(d.count.sum())
    assert r["idx"].max() < case.n_wl and r["feature"].max() < case.n_features and (r["flags"] & 0x0F).max() < case.n_libs


def test_small_case_holds_every_class():
    """the composite case: every size class at both sides of its constant, in a tile and across tile multiples"""
    case = CC.get_case("small_L12")
    d = CC.check_claims(case)
    seen = set((c["S"], c["klass"]) for c in case.claims if c["kind"] == "segment" and "klass" in c)
    T = CC.UC_TILE
    for want in ((1, "tile_small"), (2, "tile_small"), (CC.UC_SMALL, "tile_small"), (CC.UC_SMALL + 1, "tile_long"), (64, "tile_long"),
                 (T - 1, "tile_long"), (T, "tile_long"), (2, "edge_small"), (CC.UC_SMALL, "edge_small"), (CC.UC_SMALL + 1, "edge_small"),
                 (CC.UES_CAP, "edge_small"), (CC.UES_CAP + 1, "edge_large"), (CC.UE_CAP, "edge_large"), (CC.UE_CAP + 1, "giant")):
        assert want in seen, want
    kinds = set(c["kind"] for c in case.claims)
    assert {"same_tile", "abut", "parity", "hub", "column", "last_tile", "mixed_utypes"} <= kinds
    assert any(c.get("headless_tiles") for c in case.claims) and any(c.get("ends_array") for c in case.claims)
    assert sum(1 for c in case.claims if c.get("mux")) == 3 and d.n_group_keys > 0


def test_rule_segment_moves_as_written():
    """the hand-made rule segment: the moves its builder wrote down are the ones correct_umis makes"""
    for L in (11, 12, 16):
        keys, moves = CC.rule_keys(L)
        raw = {(L, k[3], 5): k[4] for k in keys}
        corr = py_correct(raw)
        assert {u: (corr[(L, u, 5)][1] if (L, u, 5) in corr else None) for u in moves} == moves
        hub_keys, hub = CC.hub_keys(L)
        corr = py_correct({(L, k[3], 5): k[4] for k in hub_keys})
        assert len(corr) == 3 * L and all(t[1] == hub for t in corr.values())


def test_translated_segments_are_the_same_reads():
    for S in CC.TRANSLATED:
        ref = None
        for off in CC.TRANSLATED_OFFSETS:
            case = CC.translation_case(S, off)
            CC.check_claims(case)
            r = case.records
            m = r["idx"] == case.segment_bc
            seg = tuple(r[k][m].tobytes() for k in ("umi", "feature", "flags", "ulen"))
            assert ref is None or seg == ref
            ref = seg


def test_collision_case_bit_patterns():
    """Both kinds of collision exist in the 64-bit layout with 250 000 keys (vbits = 18): the search through the inverse of
    mix64 took 2^20 hashes per seed for the first kind and all 2^18 top-bit patterns per seed for the second."""
    case = CC.get_case("collisions")
    d = CC.describe(case)
    n = CC.check_collisions(case, d)
    assert n[1] >= 1 and n == case.n_kind
    assert n[2] >= 1, "no pair left that only the exact group comparison separates"
    assert d.n_group_keys == 4 * (n[1] + n[2])
    assert case.key_bits == 64


@pytest.mark.parametrize("name", list(CC.SMALL_CASES))
def test_restatement_equals_the_oracle(name):
    case = CC.get_case(name)
    CC.check_claims(case)
    exp = oracle_expected(case)
    mine = CC.expected(case, py_mark)
    assert_same_results(mine, exp, name)
    assert (exp["flags"] & 1).all()
    if name == "small_L12":
        assert ((exp["flags"] & 2) != 0).sum() > 1000 and ((exp["flags"] & 4) != 0).sum() > 100
    if name == "low_support":
        assert ((exp["flags"] & 4) != 0).sum() >= 10
