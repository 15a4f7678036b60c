"""GPU parity of the feature stage on constructed boundary cases (tests/feature_cases.py): every row shape and the byte tail of
k_match_features_lds, second batches of the grid-stride loops with a planned pending-capture queue per workgroup, the staging
geometry of k_extract_tethered_lds over strides, windows and needles, the constants (FXT_MAXC, FX_LOCAL_ENTRIES, the n_feat
switches, rec_cap), the two-pass record flow, the generic kernel and its queue, and k_feature_counts past its table.  Every
case asserts its own structure (feature_cases.check_claims) before any result is compared; feature_out, n_ids_out and
capture_out are compared in full with the restatement of feature_extraction.rs:34-117, :358-470, guard elements included.
The counters say which kernel a call took."""
import time

import numpy as np
import pytest

import feature_cases as FC

pytestmark = pytest.mark.gpu

STAT_REQUEUED, STAT_FAST, STAT_RESUMED = 2, 4, 8      # crgpu.h: CRGPU_STAT_FEATURE_READS_REQUEUED, _FAST_LAUNCHES, _RESUMED_READS
GUARD, SENTINEL = 64, 0xDEADBEEF
OUTPUTS = ("feature_out", "n_ids_out", "capture_out")
timings = []


@pytest.fixture(autouse=True)
def _report_timings(monkeypatch):
    """wall time of every run of a test, context and extractor set-up apart (shown with -s)"""
    monkeypatch.delenv("CRGPU_FEATURES_GLOBAL", raising=False)
    del timings[:]
    yield
    for kind, what, t in timings:
        print("%-10s %9.3f ms  %s" % (kind, 1e3 * t, what))


def _context():
    import gpu_helpers as G

    t = time.perf_counter()
    c = G.fresh_ctx()
    timings.append(("context", "", time.perf_counter() - t))
    return c


def _stats(c):
    return np.array([c.stat(STAT_FAST), c.stat(STAT_REQUEUED), c.stat(STAT_RESUMED)], np.int64)


def _guarded(c, n):
    return c.upload(np.full(n + GUARD, SENTINEL, np.uint32))


def _same(got, exp, n, what, which):
    assert (got[n:] == SENTINEL).all(), (what, "guard")
    bad = np.nonzero(got[:n] != exp)[0]
    assert not len(bad), (what, "%d reads differ" % len(bad), "reads", bad[:6].tolist(), "rows", which[bad[:6]].tolist(),
                          "got", [hex(int(x)) for x in got[bad[:6]]], "expected", [hex(int(x)) for x in exp[bad[:6]]])


# ---- group A ------------------------------------------------------------------------------------------------------------
def _run_match(c, case, monkeypatch, env_global=False):
    d = FC.check_claims(case, env_global=env_global)
    seq, qn = case.arrays()
    n, nb = case.n, case.n * case.L
    c.set_feature_pattern(0, np.frombuffer(b"".join(case.feats), np.uint8).reshape(len(case.feats), case.L), case.index,
                          None if case.dist is None else np.array(case.dist))
    buf = np.full(case.offset + nb, 0x7F, np.uint8)
    buf[case.offset:] = qn.ravel()
    d_seq, d_q, d_out = c.upload(seq), c.upload(buf), _guarded(c, n)
    if env_global:
        monkeypatch.setenv("CRGPU_FEATURES_GLOBAL", "1")
    t = time.perf_counter()
    c.match_features(0, d_seq, d_q.ptr + case.offset, n, d_out)
    got = d_out.to_host()
    timings.append(("match", "%s n %d %s%s" % (case.name, n, d.kernel, " (CRGPU_FEATURES_GLOBAL)" if env_global else ""), time.perf_counter() - t))
    monkeypatch.delenv("CRGPU_FEATURES_GLOBAL", raising=False)
    _same(got, case.expected(), n, (case.name, d.kernel), case.which)
    for b in (d_seq, d_q, d_out):
        b.free()


@pytest.mark.parametrize("L", FC.A_LENGTHS)
def test_group_a_row_shapes(L, monkeypatch):
    """captures of L bases in calls of 1, 63, 64, 65, 255, 256 and 257 reads: the four shifts of the row assembly, its masks at
    L < 8, 8, 8 < L < 16 and 16, the byte-wise tail of the staging at n * L % 4 = 1, 2, 3; substitutions and Ns at position 0,
    on both sides of the half split and at L - 1, two Ns, every edge quality"""
    c = _context()
    for n in FC.A_SIZES:
        case = FC.get_case("a_L%d_n%d" % (L, n))
        _run_match(c, case, monkeypatch)
        _run_match(c, case, monkeypatch, env_global=True)
    c.close()


def test_group_a_posterior_switches_and_collisions(monkeypatch):
    """the decisions of the posterior (0.975 from both sides, 0 / 0, the quality cap and wrap, Ns, FXT_MAXC candidates and one
    more); 1024 / 1025 and 4096 / 4097 features; a quality array one byte off a dword (k_match_features); no distribution;
    features whose home is the last slot of 64 and of 128"""
    c = _context()
    for name in ["a_posterior", "a_unaligned", "a_no_dist", "a_wrap_32", "a_wrap_33"] + [n for n in FC.names("a") if n.startswith("a_nfeat_")]:
        case = FC.get_case(name)
        _run_match(c, case, monkeypatch)
        _run_match(c, case, monkeypatch, env_global=True)
    c.close()


@pytest.mark.parametrize("name", [n for n in FC.names("a") if n.startswith("a_grid_")])
def test_group_a_second_batch_and_queue_carry_over(name, monkeypatch):
    """one sweep of the grid, three tiles and 37 reads more: workgroup 0 drains at np == THREADS, workgroup 1 keeps THREADS - 1
    captures at the front while the newest THREADS are corrected, workgroup 2 reaches THREADS with its second batch,
    workgroup 3's second batch is short; with 1025 features the 1024-thread kernel"""
    c = _context()
    _run_match(c, FC.get_case(name), monkeypatch)
    c.close()


# ---- groups B and C -----------------------------------------------------------------------------------------------------
class _Device:
    """the rows of a case on the device"""

    def __init__(self, c, case):
        self.args, self.keep = {}, []
        for name, R in (("r1", case.r1), ("r2", case.r2)):
            if R is not None:
                s, q, ln = R.arrays(case.which)
                self.args[name] = (c.upload(s), c.upload(q), None if ln is None else c.upload(ln), R.stride)

    def free(self):
        for a in self.args.values():
            for b in a[:3]:
                if b is not None:
                    b.free()


def _call(c, case, dev, outs, extractor, with_dist, what):
    """one crgpu_extract_features_dev call; all three outputs against the restatement; returns the counters' differences"""
    before = _stats(c)
    t = time.perf_counter()
    c.extract_features(extractor, case.n, outs[0], d_n_ids_out=outs[1], d_capture_out=outs[2], **dev.args)
    got = [o.to_host() for o in outs]
    timings.append(("extract", "%s n %d %s" % (case.name, case.n, what), time.perf_counter() - t))
    delta = _stats(c) - before
    for g, e, name in zip(got, case.expected(with_dist), OUTPUTS):
        _same(g, e, case.n, (case.name, what, name), case.which)
    return dict(fast=int(delta[0]), requeued=int(delta[1]), resumed=int(delta[2])), got


def _set_extractors(c, case):
    c.set_feature_extractor(0, case.defs, None)
    c.set_feature_extractor(1, case.defs, np.array(case.dist))


def _run_extract(c, case, dev, monkeypatch, with_dist=True, env_global=False):
    """a call on fresh outputs (what an earlier call kept about other buffers cannot be resumed)"""
    d = FC.check_claims(case, with_dist=with_dist, env_global=env_global)
    outs = [_guarded(c, case.n) for _ in OUTPUTS]
    if env_global:
        monkeypatch.setenv("CRGPU_FEATURES_GLOBAL", "1")
    what = "%s%s%s" % (d.kernel, "" if with_dist else " no distribution", " (CRGPU_FEATURES_GLOBAL)" if env_global else "")
    st, got = _call(c, case, dev, outs, 1 if with_dist else 0, with_dist, what)
    monkeypatch.delenv("CRGPU_FEATURES_GLOBAL", raising=False)
    lds = d.kernel != "generic"
    assert st == dict(fast=1 if lds else 0, requeued=0 if lds else d.requeued, resumed=0), (case.name, what, st, d.requeued)
    for o in outs:
        o.free()
    return got


def _run_all(c, case, monkeypatch):
    """with the distribution, without, and both again through the generic kernel: identical outputs"""
    _set_extractors(c, case)
    dev = _Device(c, case)
    for with_dist in (True, False):
        fast = _run_extract(c, case, dev, monkeypatch, with_dist)
        slow = _run_extract(c, case, dev, monkeypatch, with_dist, env_global=True)
        for a, b, name in zip(fast, slow, OUTPUTS):
            assert np.array_equal(a, b), (case.name, with_dist, name)
    dev.free()


def test_group_b_strides_windows_and_needles(monkeypatch):
    """strides 4 to 260 under 5' anchored (wildcard and literal prefixes), 3' anchored (with and without lengths), doubly
    anchored and floating patterns: one dword per lane, one, two and more quads, the quad that starts in front of its window,
    win_lo of a wildcard prefix and of a 3' anchor, 64 and 65 window dwords, needles of 1 to 4 literals from the suffix or the
    prefix and none; lengths 0, need - 1, need, stride, above stride, and a whole pattern behind len"""
    c = _context()
    for name in [n for n in FC.names("b") if n.startswith("b_s")]:
        _run_all(c, FC.get_case(name), monkeypatch)
    c.close()


def test_group_b_sizes_and_capture_lengths(monkeypatch):
    """calls of 1 to 257 reads; captures of 1, 2, 3, 31 and 32 bases"""
    c = _context()
    for name in ["b_n%d" % n for n in FC.A_SIZES] + ["b_L%d" % L for L in FC.B_LENGTHS]:
        _run_all(c, FC.get_case(name), monkeypatch)
    c.close()


def test_group_b_floating_starts_posterior_and_switches(monkeypatch):
    """the first valid start at every byte alignment, a needle hit in front of the true start, below p_lo and behind len, two
    valid starts, the start at s_hi (odd and even win_dw); the decisions of the posterior with FXT_MAXC candidates and one
    more; 1024 / 1025 / 4096 / 4097 features; features on the last slot of the set"""
    c = _context()
    for name in ["b_floating_32", "b_floating_36", "b_posterior", "b_last_slot"] + [n for n in FC.names("b") if n.startswith("b_nfeat_")]:
        _run_all(c, FC.get_case(name), monkeypatch)
    c.close()


def test_group_b_feature_of_32_t(monkeypatch):
    """the feature whose packed value is the empty marker of the LDS set: exact, as the target of one substitution among two
    candidates and among FXT_MAXC + 1, and under an N.  The extractor takes the generic kernel."""
    c = _context()
    _run_all(c, FC.get_case("b_all_t"), monkeypatch)
    c.close()


@pytest.mark.parametrize("name", [n for n in FC.names("b") if n.startswith("b_grid_")])
def test_group_b_second_batch_prefetch_and_queue_carry_over(name, monkeypatch):
    """the plan of group A's grid case for k_extract_tethered_lds: rows of 16 bytes (one quad, prefetched), 32 (two quads,
    prefetched) and 64 (four quads, no prefetch), and the 1024-thread kernel; with the distribution, through the generic
    kernel, and in the two-pass flow, where the second call corrects exactly the planned captures from the records"""
    case = FC.get_case(name)
    c = _context()
    _set_extractors(c, case)
    dev = _Device(c, case)
    fast = _run_extract(c, case, dev, monkeypatch, True)
    slow = _run_extract(c, case, dev, monkeypatch, True, env_global=True)
    for a, b, what in zip(fast, slow, OUTPUTS):
        assert np.array_equal(a, b), (name, what)
    d = FC.check_claims(case, with_dist=False, recording=True)
    outs = [_guarded(c, case.n) for _ in OUTPUTS]
    st, _ = _call(c, case, dev, outs, 0, False, "recording")
    assert st == dict(fast=1, requeued=0, resumed=0), st
    st, _ = _call(c, case, dev, outs, 1, True, "from the records")
    assert st == dict(fast=1, requeued=0, resumed=d.n_pending), (st, d.n_pending)
    dev.free()
    c.close()


def test_group_b_two_pass_record_flow(monkeypatch):
    """4095 reads record nothing, 4096 do; exactly rec_cap captures without an exact feature are resumed, rec_cap + 1 are not
    (the second call reads the rows) -- equal answers; two Ns are not recorded; other output buffers do not resume"""
    c = _context()
    n0 = FC.REC_MIN_N
    for name, resumed in (("b_two_pass_%d_100" % (n0 - 1), 0), ("b_two_pass_%d_%d" % (n0, FC.rec_cap(n0)), FC.rec_cap(n0)),
                          ("b_two_pass_%d_%d" % (n0, FC.rec_cap(n0) + 1), 0)):
        case = FC.get_case(name)
        d = FC.check_claims(case, with_dist=False, recording=True)
        assert d.n_pending == int(np.isin(case.which, [1, 2, 3]).sum()) and int((case.which == 4).sum()) == 5
        _set_extractors(c, case)
        dev = _Device(c, case)
        outs, others = [_guarded(c, case.n) for _ in OUTPUTS], [_guarded(c, case.n) for _ in OUTPUTS]
        st, _ = _call(c, case, dev, outs, 0, False, "recording")
        assert st == dict(fast=1, requeued=0, resumed=0), (name, st)
        st, _ = _call(c, case, dev, others, 1, True, "other outputs")
        assert st == dict(fast=1, requeued=0, resumed=0), (name, st)
        st, a = _call(c, case, dev, outs, 1, True, "same outputs")
        assert st == dict(fast=1, requeued=0, resumed=resumed), (name, st)
        st, _ = _call(c, case, dev, outs, 1, True, "same outputs again")       # the records were used up
        assert st == dict(fast=1, requeued=0, resumed=0), (name, st)
        dev.free()
    c.close()


def test_group_c_generic_kernel_and_its_queue(monkeypatch):
    """maps of exactly FX_LOCAL_ENTRIES and FX_LOCAL_ENTRIES + 1 features (the second pattern of a read overflowing alone),
    replacement by a better second capture, windows one base apart, ties of (length, index) between patterns on both reads,
    bare captures of 1, 2, 3 and 32 bases, len < L, len == L, len above an odd stride"""
    c = _context()
    for name in FC.names("c"):
        case = FC.get_case(name)
        _set_extractors(c, case)
        dev = _Device(c, case)
        for with_dist in (True, False):
            _run_extract(c, case, dev, monkeypatch, with_dist)
        dev.free()
    c.close()


# ---- group D ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FC.names("d"))
def test_group_d_feature_counts(name):
    """more features on one home slot than probes; 13 sweeps of the grid with more distinct features per workgroup than the
    table may hold; NO_FEATURE and n_features skipped, n_features - 1 counted; counts that are not zero on entry; one read"""
    case = FC.get_case(name)
    FC.check_claims(case)
    c = _context()
    d_f = c.upload(case.feature)
    counts = case.counts_in.copy()
    t = time.perf_counter()
    got = c.feature_counts(d_f, case.n, case.n_features, counts)
    timings.append(("counts", "%s n %d" % (name, case.n), time.perf_counter() - t))
    assert got is counts and np.array_equal(counts, case.expected()), name
    assert int(counts.sum() - case.counts_in.sum()) == int((case.feature < case.n_features).sum())
    d_f.free()
    c.close()
