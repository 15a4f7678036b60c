"""GPU parity of the barcode stage on constructed boundary cases (tests/barcode_cases.py): the long bins of the exact lookup,
the 31/32 bucket switch, k_match, the hit fields of the LDS table at cnt_max and on their wraps, per-wave regions exactly
full and one over, the acceptance test of pass B at its equalities on all three pass-B paths, and the wave bookkeeping of
k_correct_sorted and k_correct_records.  Every case asserts its own structure (barcode_cases.check_claims) before any result
is compared; all reads, both tables in full, and the guard elements behind every output are compared with the restatement
of corrector.rs:111-165.  The counters say which path a call took."""
import time

import numpy as np
import pytest

import barcode_cases as BC

pytestmark = pytest.mark.gpu

STAT_K1_SPLIT_ROUNDS, STAT_MISS_RECORD_SETS, STAT_K2_SORTED_READS, STAT_K2_RECORD_READS = 3, 11, 16, 17   # crgpu.h
NOT_READ_BACK = (1 << 64) - 1      # CRGPU_STAT_K2_RECORD_READS where CORRECTED is counted by atomics
ENV = ("CRGPU_HOT_MIN_READS", "CRGPU_K1_SPLIT", "CRGPU_COLD_CAP", "CRGPU_MISS_RECORD_CAP", "CRGPU_K2_SORTED", "CRGPU_NO_MISS_RECORDS")
GUARD = 64
SENTINEL_IDX, SENTINEL_BYTE = 0xDEADBEEF, 0xA5
timings = []


@pytest.fixture(autouse=True)
def _report_timings():
    """wall time of every run of a test, set_whitelist apart (shown with -s)"""
    del timings[:]
    yield
    for kind, what, t in timings:
        print("%-14s %8.3f s  %s" % (kind, t, what))


def _context(case):
    """a fresh context with the case's lists; the time set_whitelist took is kept apart from the runs"""
    import gpu_helpers as G

    c = G.fresh_ctx(dense=False)
    t = time.perf_counter()
    for l, (keys, tr) in sorted(case.libs.items()):
        c.set_whitelist(l, keys, canon=case.canon, translate_to=tr, length=case.L)
    c.synchronize()
    timings.append(("set_whitelist", case.name, time.perf_counter() - t))
    _, canon_sorted = c.canon_order()
    assert np.array_equal(canon_sorted, case.canon)      # a rank is a position in case.canon
    return c


def _run(c, case, monkeypatch, env=None):
    """pass A and pass B of the case on the device against the restatement; returns the counters"""
    from cellranger_amd._lib import COUNTS_CORRECTED, COUNTS_PRIOR, COUNTS_VALID

    exp = BC.expected(case)
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    env = dict(case.env, **(env or {}))
    if case.hot:
        env.setdefault("CRGPU_HOT_MIN_READS", "1")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    t = time.perf_counter()
    c.reset_counts()
    if case.prior is not None:
        c.set_counts(0, COUNTS_PRIOR, case.prior)
    c.set_posterior(case.max_expected, case.thresh)
    n = case.n
    d_cb, d_q, d_fl = c.upload(case.cb), c.upload(case.qualn), c.upload(case.flags)
    d_idx = c.upload(np.full(n + GUARD, SENTINEL_IDX, np.uint32))
    d_corr = c.upload(np.full(n + GUARD, SENTINEL_BYTE, np.uint8))
    rounds_before = c.stat(STAT_K1_SPLIT_ROUNDS)      # (counted since the context was made)
    c.match_and_count(d_cb, d_fl, n, d_idx)
    idx_a = d_idx.to_host()
    st = dict(split_rounds=c.stat(STAT_K1_SPLIT_ROUNDS) - rounds_before, record_sets=c.stat(STAT_MISS_RECORD_SETS))
    valid = {l: c.get_counts(l, COUNTS_VALID) for l in case.libs}
    c.correct(d_cb, d_q, d_fl, n, d_idx, d_corr)
    idx_b, corr = d_idx.to_host(), d_corr.to_host()
    st.update(sorted_reads=c.stat(STAT_K2_SORTED_READS), record_reads=c.stat(STAT_K2_RECORD_READS), record_sets_after=c.stat(STAT_MISS_RECORD_SETS))
    corrected = {l: c.get_counts(l, COUNTS_CORRECTED) for l in case.libs}
    timings.append(("run", "%s %s" % (case.name, sorted(env.items())), time.perf_counter() - t))
    what = "%s %r max_expected %r thresh %r" % (case.name, env, case.max_expected, case.thresh)
    assert (idx_a[n:] == SENTINEL_IDX).all() and (idx_b[n:] == SENTINEL_IDX).all() and (corr[n:] == SENTINEL_BYTE).all(), what
    assert np.array_equal(idx_a[:n], exp.idx_a), what
    assert np.array_equal(idx_b[:n], exp.idx_b), what
    assert np.array_equal(corr[:n], exp.corrected), what
    for l in case.libs:
        assert np.array_equal(valid[l], exp.valid[l]), what
        assert np.array_equal(corrected[l], exp.corrected_hist[l]), what
    assert np.array_equal(valid[min(case.libs)], c.get_counts(min(case.libs), COUNTS_VALID))       # pass B leaves VALID alone
    for b in (d_cb, d_q, d_fl, d_idx, d_corr):
        b.free()
    return st


def _path(st, d, path, staged=True, overflow=False):
    """the counters of a call with a table say that pass B took `path`"""
    total = 0 if overflow else len(d.sorted_keys)
    assert st["record_sets"] == 1 and st["record_sets_after"] == 0
    if path == "sorted":
        assert st["sorted_reads"] == total and st["record_reads"] == 0
    else:
        assert st["sorted_reads"] == 0 and st["record_reads"] == (total if staged else NOT_READ_BACK)


def _scan(st):
    assert st["record_sets"] == 0 and st["sorted_reads"] == 0 and st["record_reads"] == 0


def test_group_a_exact_lookup_and_staging(monkeypatch):
    """Bins of 1, 7, 8, 9 and more keys at odd and even offsets, the last bin ending the table with the all-T key (wl_lookup,
    k_match_binned, the cold queue of k_lookup_hot); 5 and 16 bases; one barcode in every read with n a multiple of MB_TILE and
    one more (a staging region filled to its last entry); lists of 31 x 32768 and one more barcode with a table."""
    for name in ("clustered_L16", "clustered_L5", "clustered_L16_table", "one_barcode_full", "one_barcode_plus_one",
                 "bucket_switch_31", "bucket_switch_32"):
        case = BC.get_case(name)
        d = BC.check_claims(case)
        c = _context(case)
        st = _run(c, case, monkeypatch)
        if case.hot:
            _path(st, d, "records", staged=d.buckets_per_lib <= BC.SI_MISS_BUCKET)
            assert st["split_rounds"] == 0          # too few reads for counted rounds: every round staged in full
        else:
            _scan(st)
        c.close()


def test_group_b_plain_atomics_with_many_buckets(monkeypatch):
    """fifteen libraries on a canonical list of 69 x 32768 barcodes: more buckets than MB_MAX_BUCKETS, k_match<false>; reads
    with N and reads of a library without a list"""
    case = BC.get_case("many_buckets")
    BC.check_claims(case)
    c = _context(case)
    _scan(_run(c, case, monkeypatch))
    c.close()


@pytest.mark.parametrize("name", ["table_odd", "table_full"])
def test_group_c_hit_fields_of_the_table(name, monkeypatch):
    """2^20 - 1 and 2^20 barcodes: hit fields of 12 and 11 bits.  One barcode with exactly cnt_max, cnt_max + 1, cnt_max + 2 hits
    and two whole fields in one workgroup each; the top rank (rank_mask - 1 on the odd list) in most reads; five barcodes on
    four slots.  Default mode (counters in the entries), the slot stream, and every round staged in full."""
    case = BC.get_case(name)
    d = BC.check_claims(case)
    c = _context(case)
    for split, rounds in ((None, 1), ("1", 1), ("0", 0)):
        st = _run(c, case, monkeypatch, {} if split is None else {"CRGPU_K1_SPLIT": split})
        assert st["split_rounds"] == rounds, (name, split, st)
        _path(st, d, "records", staged=False)
    c.close()


def test_group_d_regions_exactly_full_and_one_over(monkeypatch):
    """CRGPU_MISS_RECORD_CAP = c with c and c + 1 misses in one wave: the exact fill keeps the records (both records paths), the
    surplus falls back to the scan.  CRGPU_COLD_CAP = c with c and c + 1 cold hits in one wave, in both table modes."""
    for name, overflow in (("record_cap_exact", False), ("record_cap_plus_one", True)):
        case = BC.get_case(name)
        d = BC.check_claims(case)
        c = _context(case)
        for k2 in ("0", "1"):
            st = _run(c, case, monkeypatch, {"CRGPU_K2_SORTED": k2})
            _path(st, d, "sorted" if k2 == "1" else "records", overflow=overflow)
            assert overflow or st["sorted_reads"] + st["record_reads"] == int(d.rec_count.sum()) > 0
        c.close()
    c = None
    for name in ("table_cold_exact", "table_cold_plus_one"):
        case = BC.get_case(name)
        d = BC.check_claims(case)
        c = c or _context(case)            # the two cases share their list
        for split in (None, "1"):
            st = _run(c, case, monkeypatch, {} if split is None else {"CRGPU_K1_SPLIT": split})
            assert st["split_rounds"] == 1
            _path(st, d, "records", staged=False)
        c.reset_counts()
    c.close()


@pytest.mark.parametrize("name", ["decision", "decision_translated"])
def test_group_e_the_decision_on_every_path(name, monkeypatch):
    """ties, ratios equal to the threshold and one ulp above, the veto at equality and one ulp above, the quality cap, priors 0, 1
    and 2^32 - 1, thresholds 1, above 1 and NaN, max_expected 0 and negative, one and two Ns, an N read and an A read on one
    key, all 48 neighbours: by the scan, from the records, in barcode order, and through the host entry points without qualities"""
    import test_barcode_cases_host as H

    case = BC.get_case(name)
    d = BC.check_claims(case)
    c = _context(case)
    for what, v in H.variants(case):
        v.hot = False
        _scan(_run(c, v, monkeypatch))
        v.hot = True
        for k2 in ("0", "1"):
            st = _run(c, v, monkeypatch, {"CRGPU_K2_SORTED": k2})
            if v.thresh != v.thresh:
                # a NaN threshold corrects nothing, on no path; the flags are cleared and the records used up all the same
                assert st["sorted_reads"] == st["record_reads"] == 0 and st["record_sets"] == 1 and st["record_sets_after"] == 0
            else:
                _path(st, d, "sorted" if k2 == "1" else "records")
    # without qualities: every base weighs BC_MAX_QV, the expected-error sum is 0.0
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    seqs, _ = case.ascii()
    for what, v in H.variants(case):
        exp = BC.expected(v, no_qual=True)
        c.reset_counts()
        c.set_counts(0, 2, case.prior)     # COUNTS_PRIOR
        c.set_posterior(v.max_expected, v.thresh)
        idx = c.match_and_count_host(0, seqs, None)
        assert np.array_equal(idx, exp.idx_a), what
        idx2, flag = c.correct_host(0, seqs, None, idx)
        assert np.array_equal(idx2, exp.idx_b) and np.array_equal(flag, exp.corrected), what
        assert np.array_equal(c.get_counts(0, 1), exp.corrected_hist[0]), what
    c.close()


def test_group_f_barcode_order_bookkeeping(monkeypatch):
    """k_correct_sorted: runs of 1, 63, 64, 65 equal keys from lanes 0 and 63, chunks of KS_HEADS, KS_HEADS + 1 and 64 runs, runs
    headed by records without an index, a batch without a usable lane, a run that disagrees on its winner, bins of 0 to 9 entries
    at both parities in both tables, more than 64 search items, 1, 64 and 65 records in all"""
    import test_barcode_cases_host as H

    for name in ("sorted", "sorted_total_1", "sorted_total_64", "sorted_total_65", "dense8"):
        case = BC.get_case(name)
        d = BC.check_claims(case)
        c = _context(case)
        for what, v in H.variants(case):
            st = _run(c, v, monkeypatch)
            _path(st, d, "sorted")
            assert st["sorted_reads"] == len(d.sorted_keys) > 0
        c.close()


@pytest.mark.parametrize("name", ["records_31", "records_32", "records_big"])
def test_group_g_record_order_bookkeeping(name, monkeypatch):
    """k_correct_records: regions of 1, 3, 4, 5, 256 and 257 records (empty parts), 63 and exactly 64 N reads in the queue of one
    wave, N reads among plain misses; CORRECTED through the staged histogram (31 buckets) and by atomics (32); records_big: 5.6 M
    reads, the smallest call in which a region holds enough records for 65 and 127 N reads in one wave's queue"""
    case = BC.get_case(name)
    d = BC.check_claims(case)
    c = _context(case)
    _path(_run(c, case, monkeypatch), d, "records", staged=name != "records_32")
    c.close()
