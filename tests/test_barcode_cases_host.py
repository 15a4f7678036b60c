"""The constructed barcode-stage cases (tests/barcode_cases.py) on the host: every case has the structure it claims, and the
Python restatement of Posterior::correct_barcode the expectations come from agrees with the project's oracle on every read
and both histograms of every case, and with the reference's own test vectors.  No device."""
import json
import os

import numpy as np
import pytest

import barcode_cases as BC

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def oracle_results(case, no_qual=False):
    """idx after pass A and pass B, corrected bytes and the histograms of every configured library, from the oracle:
    run_pipeline, or posterior_correct per miss where the case installs a PRIOR table or runs without qualities"""
    import oracle_lib as O

    L, nc = case.L, len(case.canon)
    wls = [None] * BC.MAX_LIB
    for l, (keys, tr) in case.libs.items():
        wls[l] = O.Whitelist(BC.unpack(keys, L), None if tr is None else BC.unpack(case.canon[tr], L))
    seqs, quals = case.ascii()
    reads = dict(cb=seqs, cb_qual=quals, lib=(case.flags & BC.FLAG_LIB_MASK).astype(np.uint8))
    res = O.run_pipeline(reads, wls, count=False, max_expected_errors=case.max_expected, threshold=case.thresh, n_threads=4)

    def ranks(ascii_seqs):
        k = BC.pack(ascii_seqs)
        r = np.searchsorted(case.canon, k)
        assert (case.canon[np.minimum(r, nc - 1)] == k).all()
        return r.astype(np.uint32)

    def table(hist):
        s, cnt = hist.dump_sorted(L)
        out = np.zeros(nc, np.uint32)
        if len(cnt):
            out[ranks(s)] = cnt.astype(np.uint32)
        return out
    out = BC.Expected()
    out.idx_a = np.full(case.n, BC.MISS, np.uint32)
    hit = res.bc_state == 1
    out.idx_a[hit] = ranks(res.corrected_cb[hit])
    out.valid = {l: table(res.valid_hist[l]) for l in case.libs}
    out.idx_b = out.idx_a.copy()
    out.corrected = np.zeros(case.n, np.uint8)
    if case.prior is None and not no_qual:
        fixed = res.bc_state == 2
        out.idx_b[fixed] = ranks(res.corrected_cb[fixed])
        out.corrected[fixed] = 1
        out.corrected_hist = {l: table(res.corrected_hist[l]) for l in case.libs}
        return out
    assert list(case.libs) == [0]
    prior = case.prior if case.prior is not None else out.valid[0]
    hist = O.Hist()
    for r in np.nonzero(prior)[0]:
        hist.observe_by(BC.seq_of(int(case.canon[r]), L), int(prior[r]))
    for i in np.nonzero(~hit & ((case.flags & BC.FLAG_LIB_MASK) == 0))[0]:
        got = O.posterior_correct(wls[0], hist, seqs[i].tobytes(), None if no_qual else quals[i], case.max_expected, case.thresh)
        if got is not None:
            out.idx_b[i] = ranks(np.frombuffer(got, np.uint8)[None, :])[0]
            out.corrected[i] = 1
    out.corrected_hist = {0: np.bincount(out.idx_b[out.corrected == 1].astype(np.int64), minlength=nc).astype(np.uint32)}
    return out


def assert_same(got, exp, what):
    assert np.array_equal(got.idx_a, exp.idx_a), "%s: idx after pass A" % what
    assert np.array_equal(got.idx_b, exp.idx_b), "%s: idx after pass B" % what
    assert np.array_equal(got.corrected, exp.corrected), "%s: corrected bytes" % what
    assert sorted(got.valid) == sorted(exp.valid)
    for l in exp.valid:
        assert np.array_equal(got.valid[l], exp.valid[l]), "%s: VALID of library %d" % (what, l)
        assert np.array_equal(got.corrected_hist[l], exp.corrected_hist[l]), "%s: CORRECTED of library %d" % (what, l)


def variants(case):
    """the parameter sets a case is run with: its own, and for the decision cases the equalities of group E"""
    if case.name.startswith("decision"):
        return [(name, case.with_params(me, th)) for name, me, th in BC.decision_params(case)]
    if case.name == "sorted":
        return [("default", case), ("veto_on", case.with_params(5.0, 0.6))]
    return [("default", case)]


def test_constants_come_from_the_source():
    assert BC.MB_TILE == 256 * BC.K["MB_ITEMS"] and BC.LH_CHUNK == BC.LH_THREADS * BC.LH_ITEMS
    assert BC.N_TABLE == BC.K["HOT_MIN_TILES"] * BC.MB_TILE and BC.first_of(BC.N_TABLE) == BC.MB_TILE
    # the counted rounds: plan.cap / REGIONS > COLD_MIN_PER_REGION, on either side of the smallest such call
    for n, counted in ((BC.N_COUNTED_MIN - 1, False), (BC.N_COUNTED_MIN, True), (BC.N_COUNTED, True)):
        cap = (n + BC.MB_TILE - 1) // BC.MB_TILE * BC.MB_TILE
        assert (cap // BC.REGIONS > BC.K["COLD_MIN_PER_REGION"]) == counted
    assert BC.cnt_shift_of((1 << 20) - 1) == 20 and BC.cnt_shift_of(1 << 20) == 21


@pytest.mark.parametrize("name", list(BC.BUILDERS))
def test_case_has_the_structure_it_claims(name):
    BC.check_claims(BC.get_case(name))


@pytest.mark.parametrize("name", list(BC.BUILDERS))
def test_restatement_equals_the_oracle(name):
    """every read, both histograms, every parameter set; a disagreement is settled against corrector.rs:111-165"""
    case = BC.get_case(name)
    for what, c in variants(case):
        assert_same(BC.expected(c), oracle_results(c), "%s / %s" % (name, what))
    if name.startswith("decision"):
        for what, c in variants(case)[:2] + variants(case)[6:8]:
            assert_same(BC.expected(c, no_qual=True), oracle_results(c, no_qual=True), "%s / %s without qualities" % (name, what))


def test_decision_runs_decide_what_they_are_named_for():
    """the equalities of group E flip exactly the read they are made of"""
    case = BC.get_case("decision")
    at = case.at
    by = {name: BC.expected(c) for name, c in variants(case)}
    hi, lo = sorted(r for _, r in BC.candidates(case, at["tie2"]))[::-1]
    assert by["tie_at_half"].idx_b[at["tie2"]] == hi and by["tie_above_half"].idx_b[at["tie2"]] == BC.MISS
    assert by["tie_at_half"].idx_b[at["tie2_rev"]] == max(r for _, r in BC.candidates(case, at["tie2_rev"]))
    for q in (66, 67, 127):       # capped: a tie, the larger rank; 65 weighs more than 66
        assert by["tie_at_half"].idx_b[at["cap%d" % q]] == max(r for _, r in BC.candidates(case, at["cap66"]))
    assert by["tie_at_half"].idx_b[at["cap65"]] == dict(BC.candidates(case, at["cap65"]))[5 * 4 + ((BC.get_base(int(case.cb[at["cap65"]]), 16, 5) + 1) & 3)]
    assert by["ratio_equal"].corrected[at["ratio3"]] == 1 and by["ratio_above"].corrected[at["ratio3"]] == 0
    assert by["veto_equal"].corrected[at["cap67"]] == 0 and by["veto_above"].corrected[at["cap67"]] == 1
    assert by["veto_equal"].corrected[at["cap127"]] == 1 and by["veto_above"].corrected[at["cap66"]] == 0
    assert by["thresh_one"].corrected[at["lone"]] == 1 and by["thresh_one"].corrected[at["n1_last"]] == 1
    assert by["thresh_one"].corrected[at["tie2"]] == 0
    for name in ("thresh_above_one", "thresh_nan", "max_expected_zero", "max_expected_negative"):
        assert by[name].corrected.sum() == 0, name
    assert by["veto_on_lone"].corrected[at["lone"]] == 1 and by["veto_on_lone"].corrected[at["lone_q34"]] == 1
    assert by["tie_at_half"].corrected[at["n4_first"]] == 1 and by["tie_at_half"].corrected[at["n_two"]] == 0
    assert by["tie_at_half"].corrected[at["n0_first"]] == 0 and by["tie_at_half"].idx_b[at["same_key_a"]] != by["tie_at_half"].idx_b[at["same_key_n"]]
    # the translated list: the tie goes to the larger canonical sequence, which is the smaller raw one
    tc = BC.get_case("decision_translated")
    e = BC.expected(tc.with_params(BC.DBL_MAX, 0.5))
    assert e.idx_b[tc.at["tie2"]] == max(r for _, r in BC.candidates(tc, tc.at["tie2"]))


def test_restatement_reproduces_the_reference_vectors():
    """the `posterior` blocks of corrector_vectors.json (corrector.rs:196-313)"""
    with open(os.path.join(GOLD, "corrector_vectors.json")) as f:
        blocks = json.load(f)["posterior"]
    assert blocks
    for b in blocks:
        wl = set(s.encode() for s in b["whitelist"])
        counts = {k.encode(): v for k, v in b["bc_counts"].items()}
        for c in b["cases"]:
            got = BC.correct_barcode(c["seq"].encode(), c["qual"], lambda s: s if s in wl else None, lambda s: counts.get(s, 0),
                                     b["max_expected_barcode_errors"], b["bc_confidence_threshold"])
            assert got == (None if c["expect"] is None else c["expect"].encode()), (b["name"], c)
