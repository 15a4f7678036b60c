"""GPU parity of the read ingest on constructed edge cases (tests/ingest_cases.py), exact against plain restatements: FASTQ
text -> rows with line feeds and CR/LF pairs on every tile and round edge, the grid wrap and the cap of 4096 workgroups, the
refusals; pack / pack_rows / pack_rows_var at every length, offset and byte value and beyond the grid wrap; the shard
metrics at all 256 length pairs; the whole-read metrics and the homopolymer windows.  Every case asserts its own structure
before any result is compared.  Every output buffer is filled with a sentinel and has a guard behind it (one more row, or 64
more elements) that must come back untouched, as must the rows between the records found and the room given; all rows are
compared, never a sample."""
import ctypes as C
import time

import numpy as np
import pytest

import ingest_cases as IC

pytestmark = pytest.mark.gpu

EINVAL, ERANGE = -1, -6
S8, S32 = 0xA5, 0xA5A5A5A5


def _ctx():
    import gpu_helpers as G

    return G.fresh_ctx()


class Guarded:
    """a device buffer of `used` elements and `guard` more, all set to the sentinel"""

    def __init__(self, c, used, guard, dtype):
        self.used, self.dtype = int(used), np.dtype(dtype)
        self.sentinel = self.dtype.type(S8 if self.dtype.itemsize == 1 else S32)
        self.fill = np.full(self.used + int(guard), self.sentinel, self.dtype)
        self.d = c.empty(len(self.fill), self.dtype)
        self.reset()

    def reset(self):
        self.d.upload(self.fill)
        return self

    def result(self, written=None, shape=None):
        """the first `written` elements; everything behind them must still be the sentinel"""
        h = self.d.to_host()
        w = self.used if written is None else int(written)
        assert (h[w:] == self.sentinel).all(), "written behind the end of the output"
        return h[:w] if shape is None else h[:w].reshape(shape)

    def untouched(self):
        return bool((self.d.to_host() == self.sentinel).all())


# ---- FASTQ ---------------------------------------------------------------------------------------------------------------------
class Fastq:
    """row buffers for max_records records and one guard row, a text buffer; the raw call, so that the count is seen on refusals"""

    def __init__(self, c, max_records, stride, text_cap, with_len=True):
        from cellranger_amd import engine as E

        self.c, self.E, self.max_records, self.stride = c, E, max_records, stride
        self.d_text = c.empty(max(text_cap, 1), np.uint8)
        self.seq = Guarded(c, max_records * stride, stride, np.uint8)
        self.qual = Guarded(c, max_records * stride, stride, np.uint8)
        self.len = Guarded(c, max_records, 64, np.uint32) if with_len else None

    def call(self, text, max_records=None, n_bytes=None):
        t = np.frombuffer(text, np.uint8) if isinstance(text, (bytes, bytearray)) else text
        if len(t):
            self.d_text.upload(t)
        for g in (self.seq, self.qual, self.len):
            if g is not None:
                g.reset()
        n = C.c_uint64(77)
        p = self.E._p
        rc = self.c.L.crgpu_fastq_to_rows_dev(self.c.h, p(self.d_text), len(t) if n_bytes is None else n_bytes, self.stride,
                                              self.max_records if max_records is None else max_records, p(self.seq.d), p(self.qual.d),
                                              p(self.len.d) if self.len else None, C.byref(n))
        return rc, n.value

    def accepted(self, text, expect=None, what=""):
        """the call takes the text and gives the restatement's rows; nothing behind the records is touched"""
        exp = IC.fastq_rows(text, self.stride) if expect is None else expect
        rc, n = self.call(text)
        assert rc == 0, "%s: refused (%d): %s" % (what, rc, (self.c.L.crgpu_last_error(self.c.h) or b"").decode())
        assert n == len(exp[2]), "%s: %d records, not %d" % (what, n, len(exp[2]))
        seq = self.seq.result(n * self.stride, (n, self.stride))
        qual = self.qual.result(n * self.stride, (n, self.stride))
        assert np.array_equal(seq, exp[0]), "%s: sequence rows" % what
        assert np.array_equal(qual, exp[1]), "%s: quality rows" % what
        if self.len:
            assert np.array_equal(self.len.result(n), exp[2]), "%s: lengths" % what
        return n

    def refused(self, text, code, what="", untouched=False, **kw):
        rc, n = self.call(text, **kw)
        assert rc == code, "%s: returned %d, not %d" % (what, rc, code)
        assert n == 0, "%s: reports %d records" % (what, n)
        for g in (self.seq, self.qual, self.len):
            g.result(g.used)                                  # the guard in any case
            if untouched:
                assert g.untouched(), what


def test_fastq_small_shapes():
    """group A: one record under 256 bytes with every line end; empty reads; quality lines that begin with '@' and '+'; reads
    of stride - 1, stride, stride + 1 and 3 x stride bases at six strides; no length output; the densest legal text"""
    c = _ctx()
    for case in IC.small_fastq_cases():
        IC.check_small_case(case)
        exp = IC.fastq_rows(case.text, case.stride)
        n = len(exp[2])
        f = Fastq(c, n + 2, case.stride, len(case.text), with_len=not getattr(case, "no_len", False))
        assert f.accepted(case.text, exp, case.name) == n
    c.close()


def test_fastq_boundaries_by_sweep():
    """group B: a text of two tiles whose first header grows by d = 0..511 bytes, with LF and CR/LF line ends, with and without
    the final one: line feeds on the last byte of a tile and the first of the next, a CR and its LF on either side of a
    tile and of a 256-byte round, lengths of a whole number of tiles and one fewer.  Plus the shortest text whose last tile
    holds a single byte."""
    c = _ctx()
    n = len(IC.sweep_records())
    for variant in IC.SWEEP_VARIANTS:
        IC.check_sweep(variant)
        f = Fastq(c, n + 3, IC.SWEEP_STRIDE, len(IC.sweep_text(variant, IC.SWEEP_D - 1)))
        for d in range(IC.SWEEP_D):
            assert f.accepted(IC.sweep_text(variant, d), None, "%s d = %d" % (variant, d)) == n
    text = IC.one_byte_tile_text()
    assert IC.describe_text(text)["len_mod_tile"] == 1
    exp = IC.fastq_rows(text, 32)
    Fastq(c, len(exp[2]) + 1, 32, len(text)).accepted(text, exp, "tile of one byte")
    c.close()


def test_fastq_grid_wrap_and_workgroup_cap():
    """group C: 8192 + 5 records in one call (the wave-per-record loop goes round), and one text just above 64 MiB (4096
    workgroups before the rounding, tiles above 4 x FQ_TILE), built by tiling a block; its reference rows are tiled alike"""
    c = _ctx()
    case = IC.wrap_fastq_case()
    IC.check_small_case(case)
    assert case.n == IC.WAVE_WRAP + 5
    Fastq(c, case.n + 2, case.stride, len(case.text)).accepted(case.text, None, "wrap")
    t0 = time.perf_counter()
    big = IC.large_fastq_case()
    plan = IC.check_large_case(big)
    t1 = time.perf_counter()
    f = Fastq(c, big.n + 1, big.stride, len(big.text))
    rc, n = f.call(big.text)
    assert rc == 0 and n == big.n
    seq, qual = f.seq.result(n * big.stride, (n, big.stride)), f.qual.result(n * big.stride, (n, big.stride))
    lens = f.len.result(n)
    t2 = time.perf_counter()
    assert np.array_equal(seq, big.seq) and np.array_equal(qual, big.qual) and np.array_equal(lens, big.lens)
    t3 = time.perf_counter()
    print("large text: %d bytes, %d records, plan %r; host reference %.3f s, device call with copies %.3f s, comparison %.3f s"
          % (len(big.text), n, plan, t1 - t0, t2 - t1, t3 - t2))
    c.close()


def test_fastq_refusals():
    """group D: line counts of 4k + 1, 2, 3; a header without '@' in the first, a middle (later tile) and the last record; a
    separator without '+'; a quality line one byte short or long in the last record; line feeds only; no room.  After every
    refusal the count is 0 and the same context takes the next good text."""
    c = _ctx()
    cases, base, n_good = IC.refusal_cases()
    good = IC.fastq_rows(base, 8)
    f = Fastq(c, n_good + 4, 8, max(len(x.text) for x in cases))
    for case in cases:
        IC.check_refusal_case(case)
        f.refused(case.text, EINVAL, case.name)
        assert f.accepted(base, good, "after " + case.name) == n_good
    f.refused(base, ERANGE, "room for n - 1", untouched=True, max_records=n_good - 1)
    assert f.accepted(base, good, "after ERANGE") == n_good
    exact = Fastq(c, n_good, 8, len(base))                    # room for exactly n
    assert exact.accepted(base, good, "room for n") == n_good
    rc, n = f.call(base, n_bytes=0)
    assert rc == 0 and n == 0 and f.seq.untouched() and f.qual.untouched() and f.len.untouched()
    c.close()


# ---- pack -------------------------------------------------------------------------------------------------------------------------
class PackOut:
    def __init__(self, c, n, L, flags_in=None, var=False):
        self.n, self.L = n, L
        self.packed, self.qualn = Guarded(c, n, 64, np.uint32), Guarded(c, n * L, L, np.uint8)
        self.flags = None
        if flags_in is not None:
            self.flags = Guarded(c, n, 64, np.uint8)
            self.flags.d.upload(np.concatenate([flags_in, self.flags.fill[n:]]))
        self.len_out = Guarded(c, n, 64, np.uint8) if var else None

    def check(self, exp, flags_in=None, what=""):
        key, qualn = self.packed.result(), self.qualn.result(shape=(self.n, self.L))
        assert np.array_equal(key, exp[0]), "%s: packed words" % what
        assert np.array_equal(qualn, exp[1]), "%s: qualn" % what
        if self.flags is not None:      # the N bit is OR-ed in, everything else stays
            assert np.array_equal(self.flags.result(), flags_in | np.where(exp[2], IC.FLAG_CB_HAS_N, 0).astype(np.uint8)), "%s: flags" % what
        if self.len_out is not None:
            assert np.array_equal(self.len_out.result(), exp[2]), "%s: lengths" % what
        return key, qualn


def _flags_in(n):
    f = (np.arange(n) % 16).astype(np.uint8) | np.uint8(0x20)
    f[::5] |= np.uint8(IC.FLAG_CB_HAS_N)                      # already set: stays set
    return f


def test_pack_every_length_offset_and_byte_value():
    """group E: lengths 1..16 of pack, and of pack_rows at offsets 0, 1, 7, stride - len and strides 31, 32, 100; the vector
    path of pack against the byte path of pack_rows at 16; every byte value at every base and quality position; flags given
    (library bits kept) and NULL; the alignment refusal; pack_rows_var at every read length; 524 288 + 301 reads each"""
    from cellranger_amd._lib import CrgpuError

    c = _ctx()
    n = 300
    seq100, qual100 = IC.pack_reads(n, 100, 510)
    fl = _flags_in(n)
    for stride in (31, 32, 100):
        rows, qrows = np.ascontiguousarray(seq100[:, :stride]), np.ascontiguousarray(qual100[:, :stride])
        d_rows, d_qrows = c.upload(rows), c.upload(qrows)
        for L in range(1, 17):
            for k, off in enumerate((0, 1, 7, stride - L)):
                exp = IC.pack_rows_ref(rows, qrows, off, L)
                assert exp[2].any() and not exp[2].all()
                o = PackOut(c, n, L, fl if k % 2 == 0 else None)
                c.pack_rows(d_rows, d_qrows, n, stride, off, L, o.packed.d, o.qualn.d, o.flags.d if o.flags else None)
                got_rows = o.check(exp, fl, "pack_rows stride %d offset %d length %d" % (stride, off, L))
            if stride == 100:
                s, q = np.ascontiguousarray(rows[:, off:off + L]), np.ascontiguousarray(qrows[:, off:off + L])
                for flags in (fl, None):
                    o = PackOut(c, n, L, flags)
                    c.pack(c.upload(s), c.upload(q), n, L, o.packed.d, o.qualn.d, o.flags.d if o.flags else None)
                    got = o.check(IC.pack_ref(s, q), fl, "pack length %d" % L)
                for a, b in zip(got, got_rows):                 # at 16: the vector path and the byte path agree
                    assert np.array_equal(a, b)
    # every byte value at every position, bases and qualities, on both paths of pack and through pack_rows
    for L in (16, 5):
        for what in ("base", "qual"):
            s, q = IC.byte_value_blocks(L, what)
            exp = IC.pack_ref(s, q)
            if what == "base":
                assert exp[2].sum() == 252 * L
            else:
                assert (exp[1] == 127).sum() == 129 * L and (exp[1] >= 128).sum() == 0
            m = len(s)
            o = PackOut(c, m, L, np.zeros(m, np.uint8))
            c.pack(c.upload(s), c.upload(q), m, L, o.packed.d, o.qualn.d, o.flags.d)
            o.check(exp, np.zeros(m, np.uint8), "pack of every %s byte, length %d" % (what, L))
            rows, qrows = np.full((m, L + 3), ord("N"), np.uint8), np.full((m, L + 3), 255, np.uint8)
            rows[:, 2:2 + L], qrows[:, 2:2 + L] = s, q
            o = PackOut(c, m, L, np.zeros(m, np.uint8))
            c.pack_rows(c.upload(rows), c.upload(qrows), m, L + 3, 2, L, o.packed.d, o.qualn.d, o.flags.d)
            o.check(exp, np.zeros(m, np.uint8), "pack_rows of every %s byte, length %d" % (what, L))
    # 16-base buffers that are not 16-byte aligned are refused, and nothing is written
    s, q = IC.pack_reads(65, 16, 511)
    d_s, d_q = c.upload(s), c.upload(q)
    o = PackOut(c, 65, 16, np.zeros(65, np.uint8))
    for shift in ((1, 0, 0), (0, 1, 0), (0, 0, 1)):
        with pytest.raises(CrgpuError) as e:
            c.pack(d_s.ptr + shift[0], d_q.ptr + shift[1], 64, 16, o.packed.d, o.qualn.d.ptr + shift[2], o.flags.d)
        assert e.value.code == EINVAL
        assert o.packed.untouched() and o.qualn.untouched() and np.array_equal(o.flags.result(), np.zeros(65, np.uint8))
    c.pack(d_s.ptr + 1, d_q.ptr + 1, 64, 15, o.packed.d, o.qualn.d.ptr + 1, None)       # 15 bases: any alignment
    exp = IC.pack_ref(s.reshape(-1)[1:961].reshape(64, 15), q.reshape(-1)[1:961].reshape(64, 15))
    assert np.array_equal(o.packed.d.to_host()[:64], exp[0]) and np.array_equal(o.qualn.d.to_host()[1:961].reshape(64, 15), exp[1])
    # pack_rows_var: every read length 0..stride + 2 at the five (offset, length, min_length)
    stride = IC.PACK_VAR_STRIDE
    rows, qrows, read_len = IC.pack_var_rows()
    d_rows, d_qrows, d_rl = c.upload(rows), c.upload(qrows), c.upload(read_len)
    for off, length, mn in IC.pack_var_triples():
        exp = IC.pack_rows_var_ref(rows, qrows, read_len, off, length, mn)
        assert set(exp[2].tolist()) == {0} | set(range(mn, length + 1))
        o = PackOut(c, len(rows), length, var=True)
        c.pack_rows_var(d_rows, d_qrows, d_rl, len(rows), stride, off, length, mn, o.packed.d, o.qualn.d, o.len_out.d)
        o.check(exp, what="pack_rows_var (%d, %d, %d)" % (off, length, mn))
    # beyond the grid: the grid-stride loops of the three kernels go round
    m = IC.THREAD_WRAP + 301
    s, q = IC.pack_reads(m, 16, 512)
    d_s, d_q = c.upload(s), c.upload(q)
    exp = IC.pack_ref(s, q)
    fl = _flags_in(m)
    o = PackOut(c, m, 16, fl)
    c.pack(d_s, d_q, m, 16, o.packed.d, o.qualn.d, o.flags.d)
    o.check(exp, fl, "pack beyond the grid")
    o = PackOut(c, m, 16, fl)
    c.pack_rows(d_s, d_q, m, 16, 0, 16, o.packed.d, o.qualn.d, o.flags.d)
    o.check(exp, fl, "pack_rows beyond the grid")
    read_len = np.random.default_rng(513).integers(0, 19, size=m).astype(np.uint32)
    o = PackOut(c, m, 16, var=True)
    c.pack_rows_var(d_s, d_q, c.upload(read_len), m, 16, 0, 16, 1, o.packed.d, o.qualn.d, o.len_out.d)
    exp = IC.pack_rows_var_ref(s, q, read_len, 0, 16, 1)
    assert set(exp[2].tolist()) == set(range(17))
    o.check(exp, what="pack_rows_var beyond the grid")
    c.close()


# ---- shard metrics ---------------------------------------------------------------------------------------------------------------
def _shard(c, cb, cbq, umi, uq, idx):
    import oracle_lib as O

    kb, qb, _ = IC.pack_ref(cb, cbq)
    ku, qu, _ = IC.pack_ref(umi, uq)
    d = [c.upload(x) for x in (kb, qb, ku, qu)]
    n = len(cb)
    got = c.shard_metrics(d[0], d[1], cb.shape[1], d[2], d[3], umi.shape[1], None, n)
    exp = O.shard_metrics(cb, cbq, umi, uq)
    assert exp["miss_whitelist_barcode"] == 0
    assert got == exp, "lengths (%d, %d), no idx: %r" % (cb.shape[1], umi.shape[1], {k: (got[k], exp[k]) for k in exp if got[k] != exp[k]})
    got = c.shard_metrics(d[0], d[1], cb.shape[1], d[2], d[3], umi.shape[1], c.upload(idx), n)
    exp = O.shard_metrics(cb, cbq, umi, uq, (idx != IC.MISS).astype(np.uint8))
    assert got == exp, "lengths (%d, %d), idx: %r" % (cb.shape[1], umi.shape[1], {k: (got[k], exp[k]) for k in exp if got[k] != exp[k]})
    for x in d:
        x.free()
    return exp


def test_shard_metrics_every_length_pair():
    """group F: all 256 pairs (cb_len, umi_len), each with the read classes of ingest_cases.shard_reads, with and without pass
    A's output, against the oracle; reads that leave ten counters at 0; 524 288 + 301 reads at (16, 12)"""
    c = _ctx()
    for a in range(1, 17):
        for b in range(1, 17):
            cb, cbq, umi, uq, classes = IC.shard_reads(a, b)
            exp = _shard(c, cb, cbq, umi, uq, IC.shard_idx(len(cb)))
            assert exp["miss_whitelist_barcode"] == (len(cb) + 2) // 3 and exp["has_n_umi"] > 0 and exp["homopolymer_barcode"] >= 5
            assert (exp["polyt_suffix_umi"] > 0) == (b >= 5)
    cb, cbq, umi, uq = IC.shard_zero_reads()
    exp = _shard(c, cb, cbq, umi, uq, np.arange(len(cb), dtype=np.uint32))
    assert all(exp[f] == 0 for f in IC.SHARD_ZERO_FIELDS) and exp["good_umi"] == len(cb)
    n = IC.THREAD_WRAP + 301
    exp = _shard(c, *IC.shard_random_reads(n, 16, 12), IC.shard_idx(n))
    assert exp["sequenced_reads"] == n and min(exp.values()) > 1000
    c.close()


# ---- whole-read metrics ------------------------------------------------------------------------------------------------------------
def test_rows_and_homopolymer_metrics():
    """group G: rows of 0, 1, 63..65, 127..129 bytes, of the stride and clamped to it, with and without lengths, 8192 + 5 rows;
    homopolymer runs at every start over three windows for nine run lengths, the near misses, the smallest rows, read pairs"""
    from cellranger_amd._lib import CrgpuError

    c = _ctx()
    stride = IC.ROWS_STRIDE
    for n_random in (0, IC.WAVE_WRAP + 5 - 10):
        seq, qual, lens = IC.rows_metrics_rows(n_random)
        n = len(seq)
        assert n == n_random + 10 and set(IC.ROWS_LENGTHS) <= set(lens[:10].tolist())
        d_seq, d_qual = c.upload(seq), c.upload(qual)
        assert c.rows_metrics(d_seq, d_qual, n, stride, c.upload(lens)) == IC.rows_metrics_ref(seq, qual, lens, stride)
        # without lengths every byte of a row counts; zero padding is a base that is neither N nor above Q2
        col = np.arange(stride)[None, :]
        seq0, qual0 = np.where(col < lens[:, None], seq, 0).astype(np.uint8), np.where(col < lens[:, None], qual, 0).astype(np.uint8)
        exp = IC.rows_metrics_ref(seq0, qual0, None, stride)
        with_len = IC.rows_metrics_ref(seq, qual, lens, stride)
        assert exp == dict(with_len, bases=n * stride)
        assert c.rows_metrics(c.upload(seq0), c.upload(qual0), n, stride, None) == exp
    assert n == IC.WAVE_WRAP + 5

    def hp(rows, lens, s1, run_len, **kw):
        return c.homopolymer_metrics(c.upload(rows), s1, len(rows), d_r1_len=None if lens is None else c.upload(lens), run_len=run_len, **kw)

    for k in IC.HP_RUN_LENS:
        for exact_end in (False, True):
            case = IC.hp_positive_case(k, exact_end)
            IC.check_hp_positive(case)
            assert hp(case.rows, case.lens, case.stride, k) == case.expect, case.name
        case = IC.hp_near_miss_case(k)
        IC.check_hp_near_miss(case)
        assert hp(case.rows, case.lens, case.stride, k) == case.expect, case.name
        rows, lens, s, exp = IC.hp_edge_rows(k)
        assert hp(rows, lens, s, k) == exp == IC.homopolymer_ref(rows, lens, s, k), "smallest rows, run length %d" % k
        short = np.full((5, k - 1), ord("T"), np.uint8)        # a stride below the run length
        assert hp(short, np.full(5, k + 3, np.uint32), k - 1, k) == dict.fromkeys("ACGT", 0)
        assert hp(short, None, k - 1, k) == dict.fromkeys("ACGT", 0)
    # read pairs: the run in R2 only, in both, in R1 only, in neither; another stride for R2; R2 without lengths
    r1, l1, r2, l2 = IC.hp_pair_case()
    s1, s2 = r1.shape[1], r2.shape[1]
    assert s1 != s2
    only1, both = IC.homopolymer_ref(r1, l1, s1, 15), IC.homopolymer_ref(r1, l1, s1, 15, r2, l2, s2)
    assert both != only1 and both != IC.homopolymer_ref(r2, l2, s2, 15) and sum(both.values()) < len(r1)
    assert hp(r1, l1, s1, 15) == only1
    assert hp(r1, l1, s1, 15, d_r2_rows=c.upload(r2), r2_stride=s2, d_r2_len=c.upload(l2)) == both
    assert hp(r1, l1, s1, 15, d_r2_rows=c.upload(r2), r2_stride=s2) == IC.homopolymer_ref(r1, l1, s1, 15, r2, None, s2) == both
    full = r2.copy()
    full[:, 30:] = full[:, 29:30]                              # behind R2's lengths the last base goes on: counts without them
    exp = IC.homopolymer_ref(r1, l1, s1, 15, full, None, s2)
    assert exp != both and hp(r1, l1, s1, 15, d_r2_rows=c.upload(full), r2_stride=s2) == exp
    assert hp(r1, l1, s1, 15, d_r2_rows=c.upload(full), r2_stride=s2, d_r2_len=c.upload(l2)) == both
    # 8192 + 5 rows: the wave-per-row loop goes round
    case = IC.hp_positive_case(15, False)
    n = IC.WAVE_WRAP + 5
    reps = n // len(case.rows) + 1
    rows, lens = np.tile(case.rows, (reps, 1))[:n], np.tile(case.lens, reps)[:n]
    exp = IC.homopolymer_ref(rows, lens, case.stride, 15)
    assert sum(exp.values()) == n and hp(rows, lens, case.stride, 15) == exp
    for bad in (1, 65, 0):
        with pytest.raises(CrgpuError) as e:
            hp(case.rows, case.lens, case.stride, bad)
        assert e.value.code == ERANGE
    c.close()
