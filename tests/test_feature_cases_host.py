"""The constructed feature-stage cases (tests/feature_cases.py) on the host: every case has the structure it claims, and the
Python restatement of correct_feature_barcode / find_closest / match_read the expectations come from agrees with the
project's oracle on every distinct row of every case (and over the whole arrays of the one-read cases), and with the
reference's own test vectors.  Nothing is compared with a tolerance.  No device."""
import json
import os

import numpy as np
import pytest

import feature_cases as FC

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RUNS = [dict(with_dist=True), dict(with_dist=False), dict(with_dist=False, recording=True), dict(env_global=True)]


def decode(cap):
    """the span of FeatureData::barcode as crgpu.h packs it -> (corrected, read, start, length) or None"""
    cap = int(cap)
    return None if cap == FC.NO_CAPTURE else (bool(cap >> 31), (cap >> 30) & 1, (cap >> 8) & 0x3FFFFF, cap & 0xFF)


def test_constants_come_from_the_source():
    assert FC.N_GRID == {(k, t): 262144 for k in ("k_match_features_lds", "k_extract_tethered_lds") for t in (256, 1024)}
    assert FC.slots_for(32) == 64 and FC.slots_for(33) == 128 and FC.slots_for(1) == 64
    assert FC.rec_cap(4096) == 3072 and FC.FC_FILL == 3072 and FC.FC_PROBES == 16
    assert (FC.FX_LOCAL_ENTRIES, FC.FXT_MAXC, FC.FM_MAX_FEATURES, FC.FXT_MAX_FEATURES) == (16, 8, 4096, 4096)
    assert FC.cr_grid(1, 256, 1024) == 1 and FC.cr_grid(262145, 256, 1024) == 1024 and FC.cr_grid(257, 256, 1024) == 2
    assert FC.key_of("T" * 32) == FC.M64 and FC.key_of("ACGN") == 0b00011000
    # the u8 wrap of the quality offset, the cap, and p_edit as the host code computes it
    assert FC.p_edit(32) == FC.p_edit(66) == FC.p_edit(67) == FC.p_edit(126) == 10.0 ** -3.3
    assert FC.p_edit(33) == 1.0 and FC.p_edit(34) == 10.0 ** -0.1 and FC.p_edit(65) == 10.0 ** -3.2


def test_group_a_covers_every_row_shape():
    """every (lane * L) & 3, every masking branch, and the byte-wise tail at every remainder"""
    assert {L & 3 for L in FC.A_LENGTHS} == {0, 1, 2, 3}
    assert any(L < 8 for L in FC.A_LENGTHS) and 8 in FC.A_LENGTHS and any(8 < L < 16 for L in FC.A_LENGTHS) and 16 in FC.A_LENGTHS
    assert {FC.describe(FC.get_case(n)).tail for n in FC.names("a") if n.startswith("a_L")} == {0, 1, 2, 3}


@pytest.mark.parametrize("name", list(FC.BUILDERS))
def test_case_has_the_structure_it_claims(name):
    case = FC.get_case(name)
    if isinstance(case, FC.ExtractCase):
        for kw in RUNS:
            FC.check_claims(case, **kw)
    else:
        FC.check_claims(case)


@pytest.mark.parametrize("name", FC.names("a"))
def test_group_a_restatement_equals_the_oracle(name):
    import oracle_lib as O

    case = FC.get_case(name)
    exp = case.row_expected()
    feat_ascii = np.frombuffer(b"".join(case.feats), np.uint8).reshape(len(case.feats), case.L)
    if case.dist is not None:
        assert np.array_equal(np.array(case.dist), O.compute_feature_dist(case.counts, np.zeros(len(case.counts), np.uint32)))
    dist = None if case.dist is None else np.array(case.dist)
    for k, (s, q) in enumerate(case.rows):
        f = O.find_closest_feature(feat_ascii, dist, s, q)
        assert (FC.NO_FEATURE if f < 0 else int(case.index[f])) == int(exp[k]), (name, k, s, list(q))


@pytest.mark.parametrize("name", FC.names("b") + FC.names("c"))
def test_rows_restatement_equals_the_oracle(name):
    """feature, n_ids, corrected flag, read, start and length of every distinct row, with and without the distribution; the
    feature of every read of the one-read cases through match_rows"""
    import oracle_lib as O

    case = FC.get_case(name)
    assert np.array_equal(np.array(case.dist), O.compute_feature_dist(case.counts, np.zeros(len(case.counts), np.uint32)))
    for with_dist in (True, False):
        ox = O.FeatureExtractor(case.defs, np.array(case.dist) if with_dist else None)
        exp = case.row_expected(with_dist)
        for k in range(case.n_rows):
            r1, q1, r2, q2 = case.row_reads(k)
            want = ox.match_read(r1, q1, r2, q2)
            feature, n_ids, cap = (int(x) for x in exp[k])
            got = decode(cap)
            what = (name, with_dist, k, r1, r2)
            if want is None:
                assert got is None and feature == FC.NO_FEATURE and n_ids == 0, what
                continue
            assert got == (want["corrected"], want["read"], want["start"], want["len"]), (what, got, want)
            assert n_ids == want["n_ids"], (what, n_ids, want)
            assert feature == (want["ids"][0] if want["n_ids"] == 1 else FC.NO_FEATURE), (what, feature, want)
        if case.r1 is None or case.r2 is None:
            R = case.r1 or case.r2
            s, q, ln = R.arrays(case.which)
            assert np.array_equal(ox.match_rows(s, q, read=0 if case.r1 else 1, lengths=ln, n_threads=4), case.expected(with_dist)[0]), (name, with_dist)
        ox.close()


@pytest.mark.parametrize("name", ["correct_feature", "correct_bare_feature"])
def test_restatement_reproduces_the_reference_vectors(name):
    """feature_extraction.rs:638-827, run as the reference's tests run them: match_read on a read that is the sequence"""
    with open(os.path.join(GOLD, "feature_vectors.json")) as f:
        g = json.load(f)[name]
    types = np.array(g["types"])
    dist = FC.compute_feature_dist(g["counts"], g["types"])
    for case in g["cases"]:
        x = FC.Extractor([(g["pattern"], g["features"][i], i, 0) for i in np.nonzero(types == case["type"])[0]], list(dist))
        feature, n_ids, cap = x.match_read(case["seq"].encode(), case["qual"].encode())
        if case["expect"] is None:
            assert feature == FC.NO_FEATURE and n_ids == 0, case
        else:
            assert n_ids == 1 and g["features"][feature] == case["expect"] and decode(cap)[0], case


def test_restatement_reproduces_the_reference_expressions_and_distribution():
    with open(os.path.join(GOLD, "feature_vectors.json")) as f:
        g = json.load(f)
    for c in g["compile_pattern"]:
        assert FC.compile_pattern(c["pattern"], c["length"]) == c["regex"], c
    assert FC.compile_bare_patterns(g["compile_bare"]["sequences"]) == g["compile_bare"]["regex"]
    d = g["feature_dist"]
    assert FC.compute_feature_dist(d["counts"], d["types"]) == d["expect"]
    assert FC.compute_feature_dist([0, 0, 0, 0]) == [0.25] * 4


def test_the_decisions_fall_where_the_cases_say():
    """the restatement's own numbers on the rows that are built around a decision"""
    case = FC.get_case("a_posterior")
    e = {t: int(x) for t, x in zip(case.tags, case.row_expected())}
    idx = {f: int(i) for f, i in zip(case.feats, case.index)}
    # 40 : 1 and 78 : 2 lie above 0.975 at equal qualities, 38 : 1 and 77 : 2 below
    assert e["ratio_40_1_eq"] != FC.NO_FEATURE and e["ratio_38_1_eq"] == FC.NO_FEATURE and e["ratio_77_2_eq"] == FC.NO_FEATURE
    # quality 33 and 34 make the edit likely enough; 32 wraps to the cap, 66, 67 and 126 sit on it: a tie; 65 is one step off
    assert e["qual_33"] != FC.NO_FEATURE and e["qual_34"] != FC.NO_FEATURE
    for q in (32, 65, 66, 67, 126):
        assert e["qual_%d" % q] == FC.NO_FEATURE, q
    for p in FC.split_positions(16):
        assert e["n_p%d" % p] == e["n_p0"] != FC.NO_FEATURE
    assert e["n_on_a"] == idx[case.rows[case.tags["n_on_a"]][0].replace(b"N", b"A")]
    assert e["n_four"] != FC.NO_FEATURE and e["cand8"] != FC.NO_FEATURE and e["cand9"] != FC.NO_FEATURE
    # without a distribution only the exact captures are answered
    nd = FC.MatchCase("nd", case.L, case.feats, case.index, None, case.rows, case.which).row_expected()
    assert {t for t, x in zip(case.tags, nd) if x != FC.NO_FEATURE} == {"exact", "exact_low_quality"}
