"""Constructed inputs for the barcode stage: whitelists and reads that sit on chosen sides of the boundaries of pass A
(exact lookup, LDS table of frequent barcodes, per-wave regions) and pass B (posterior correction by scan, from the miss
records, in barcode order) in barcode.hip / wl_view.h.

Host only: numpy, no device, no oracle.  The constants the cases turn on are read out of the source text, so a changed tile
size moves the cases with it.  A case is the whitelists, the packed reads, the parameters of the posterior and a list of
claims about its own structure; describe() recomputes the structure (where pass A puts a read, which record it becomes, where
the record lands once sorted, which bin a key falls into) from the arrays alone and check_claims() asserts every claim.

Expected results come from correct_barcode(), a plain restatement of Posterior::correct_barcode (barcode/src/corrector.rs:
111-165) in Python floats: candidates in position-major A<C<G<T order, max on (likelihood, sequence), exact membership for
pass A.  Nothing is compared with a tolerance."""
import math
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MISS = 0xFFFFFFFF
FLAG_LIB_MASK, FLAG_HAS_N = 0x0F, 0x10
MAX_LIB = 16
DBL_MAX = float(np.finfo(np.float64).max)
BC_MAX_QV = 66
U32 = np.uint32
ACGT = np.frombuffer(b"ACGT", np.uint8)


# ---- constants from the source ------------------------------------------------------------------------------------------
def _source(name):
    with open(os.path.join(ROOT, "cellranger_amd", "csrc", name)) as f:
        return f.read()


def _define(text, name, where):
    m = re.search(r"^#define\s+%s\s+\(?\s*(0x[0-9a-fA-F]+|\d+)u?\s*\)?\s*(?://.*)?$" % name, text, re.M)
    if not m:
        raise RuntimeError("barcode_cases: #define %s not found in %s" % (name, where))
    return int(m.group(1), 0)


def _find(text, pattern, what, where):
    m = re.search(pattern, text)
    if not m:
        raise RuntimeError("barcode_cases: %s not found in %s" % (what, where))
    return m


def _read_constants():
    bc, wv, wl = _source("barcode.hip"), _source("wl_view.h"), _source("whitelist.hip")
    k = {}
    for name in ("MB_ITEMS", "MB_MAX_BUCKETS", "BIN_SHIFT", "SI_MISS_BUCKET", "LH_THREADS", "LH_ITEMS", "HOT_SLOTS", "HOT_CAP",
                 "HC_MAX_RANK_BITS", "KS_WAVES", "KS_HEADS", "K2_PARTS", "K2_SCAN_DWORDS"):
        k[name] = _define(bc, name, "barcode.hip")
    _find(bc, r"#define\s+MB_TILE\s+\(256\s*\*\s*MB_ITEMS\)", "MB_TILE = 256 * MB_ITEMS", "barcode.hip")
    k["MB_TILE"] = 256 * k["MB_ITEMS"]
    m = _find(bc, r"hot_hash\(uint32_t key\)\s*\{\s*return \(key \* (0x[0-9a-fA-F]+)u\) >> (\d+);", "hot_hash", "barcode.hip")
    k["HOT_MUL"], k["HOT_SHIFT"] = int(m.group(1), 16), int(m.group(2))
    _find(bc, r"b1 = \(b0 \+ 1u\) & \(HOT_BUCKETS - 1u\)", "the second bucket of a key", "barcode.hip")
    _find(bc, r"#define\s+HOT_BUCKETS\s+\(HOT_SLOTS / 2u\)", "HOT_BUCKETS", "barcode.hip")
    k["K2_SORTED_MIN"] = 1 << int(_find(bc, r"sorted = sorted && ctx->n_canon > \(1u << (\d+)\)", "the list size of the barcode-order path",
                                        "barcode.hip").group(1))
    k["HOT_MIN_TILES"] = int(_find(bc, r"n >= hot_min && n >= (\d+)ull \* MB_TILE", "the smallest call with a table", "barcode.hip").group(1))
    k["COLD_MIN_PER_REGION"] = int(_find(bc, r"per_region > (\d+) \?", "the per_region condition of the counted rounds", "barcode.hip").group(1))
    m = _find(bc, r"first = n / (\d+) < \((\d+)ull << 20\) \? n / \1 : \(\2ull << 20\);\s*first = first / MB_TILE \* MB_TILE;",
              "the sampling batch", "barcode.hip")
    k["FIRST_DIV"], k["FIRST_MAX"] = int(m.group(1)), int(m.group(2)) << 20
    _find(bc, r"while \(cnt_shift < 32u && \(1ull << cnt_shift\) <= ctx->n_canon\) cnt_shift\+\+;", "the cnt_shift rule", "barcode.hip")
    _find(bc, r"const uint32_t region = blockIdx\.x \* \(LH_THREADS / 64\) \+ \(tid >> 6\);", "the region of a wave", "barcode.hip")
    _find(bc, r"const uint32_t lh_grid = cr_grid\(\(m \+ MB_TILE - 1\) / MB_TILE, 1, 256u\);", "the lookup's grid", "barcode.hip")
    _find(bc, r"rec\.regions = 256u \* \(LH_THREADS / 64\);", "the number of record regions", "barcode.hip")
    _find(wl, r"const uint32_t hA = len / 2, hB = len - hA;", "the head/tail split hA = len / 2", "whitelist.hip")
    m = _find(wl, r"uint32_t bitsE = cr_ceil_log2\(m\) > 0 \? cr_ceil_log2\(m\) - 1 : 0;\s*if \(bitsE < bitsA\) bitsE = bitsA;\s*"
                  r"if \(bitsE > key_bits\) bitsE = key_bits;\s*if \(bitsE > (\d+)\) bitsE = \1;", "the bitsE rule", "whitelist.hip")
    k["BITS_E_MAX"] = int(m.group(1))
    _find(wv, r"if \(hi > p0 \+ 8u && found == 0xFFFFFFFFu\)", "the long-bin branch of wl_lookup", "wl_view.h")
    return k


K = _read_constants()
MB_TILE, MB_MAX_BUCKETS, BIN_SHIFT, SI_MISS_BUCKET = K["MB_TILE"], K["MB_MAX_BUCKETS"], K["BIN_SHIFT"], K["SI_MISS_BUCKET"]
LH_THREADS, LH_ITEMS, HOT_SLOTS, HOT_CAP, HC_MAX_RANK_BITS = K["LH_THREADS"], K["LH_ITEMS"], K["HOT_SLOTS"], K["HOT_CAP"], K["HC_MAX_RANK_BITS"]
KS_WAVES, KS_HEADS, K2_PARTS, K2_SCAN_DWORDS = K["KS_WAVES"], K["KS_HEADS"], K["K2_PARTS"], K["K2_SCAN_DWORDS"]
BIN_SIZE = 1 << BIN_SHIFT
LH_CHUNK = LH_THREADS * LH_ITEMS          # reads of a workgroup's chunk
LH_WAVES = LH_THREADS // 64
REGIONS = 256 * LH_WAVES                  # per-wave regions of the miss records and of the cold hits
HOT_BUCKETS = HOT_SLOTS // 2
# the smallest call whose table rounds are counted (plan.cap / REGIONS > COLD_MIN_PER_REGION, plan.cap = n rounded up to MB_TILE)
N_COUNTED_MIN = (K["COLD_MIN_PER_REGION"] + 1) * REGIONS - MB_TILE + 1
N_COUNTED = (K["COLD_MIN_PER_REGION"] + 1) * REGIONS       # ... as a multiple of MB_TILE: 528 384 reads
N_TABLE = K["HOT_MIN_TILES"] * MB_TILE                     # the smallest call with a table (and miss records): 16 384 reads


# ---- sequences ----------------------------------------------------------------------------------------------------------
def pack(seqs):
    """ASCII (n, L) uint8 -> packed uint32; N packs as A, as the pack kernels do"""
    a = np.asarray(seqs, np.uint8)
    code = np.zeros(256, np.uint32)
    code[ACGT] = np.arange(4, dtype=np.uint32)
    out = np.zeros(a.shape[0], np.uint64)
    for j in range(a.shape[1]):
        out = (out << np.uint64(2)) | code[a[:, j]].astype(np.uint64)
    return out.astype(U32)


def unpack(keys, L):
    keys = np.asarray(keys, np.uint64)
    out = np.zeros((len(keys), L), np.uint8)
    for j in range(L):
        out[:, j] = ACGT[((keys >> np.uint64(2 * (L - 1 - j))) & np.uint64(3)).astype(np.int64)]
    return out


_DIGITS = bytes.maketrans(b"ACGTN", b"01230")


def key_of(s):
    return int((s.encode() if isinstance(s, str) else bytes(s)).translate(_DIGITS), 4)


def seq_of(key, L):
    return bytes(b"ACGT"[(key >> (2 * (L - 1 - j))) & 3] for j in range(L))


def set_base(key, L, pos, base):
    sh = 2 * (L - 1 - pos)
    return (key & ~(3 << sh)) | (base << sh)


def get_base(key, L, pos):
    return (key >> (2 * (L - 1 - pos))) & 3


def neighbours(key, L):
    """the 3 L keys one substitution away, in position-major A<C<G<T order"""
    return [set_base(key, L, p, b) for p in range(L) for b in range(4) if b != get_base(key, L, p)]


def hamming(a, b, L):
    x = a ^ b
    return sum(1 for p in range(L) if (x >> (2 * p)) & 3)


# ---- the reference, restated --------------------------------------------------------------------------------------------
def probability(q):
    """corrector.rs:167-171"""
    return 10.0 ** (-(float(q) - 33.0) / 10.0)


def correct_barcode(seq, qual, lookup, count_of, max_expected, thresh):
    """Posterior::correct_barcode.  seq: bytes (may hold N); qual: sequence of quality bytes or None; lookup(bytes) -> the
    (translated) whitelist sequence or None, Whitelist::check_and_update; count_of(bytes) -> prior count of a whitelist
    sequence.  Returns the corrected sequence or None."""
    a = bytearray(seq)
    best = None
    total = 0.0
    for pos in range(len(a)):
        qv = BC_MAX_QV if qual is None else min(int(qual[pos]), BC_MAX_QV)
        existing = a[pos]
        for val in b"ACGT":
            if val == existing:
                continue
            a[pos] = val
            hit = lookup(bytes(a))
            if hit is not None:
                likelihood = probability(qv) * float(1 + count_of(hit))
                cand = (likelihood, hit)
                best = cand if best is None else max(best, cand)
                total += likelihood
        a[pos] = existing
    if thresh != thresh:  # NotNan::try_from(threshold).ok()?
        return None
    expected = 0.0
    if qual is not None:
        for q in qual:
            expected += probability(int(q))
    if best is not None and expected < max_expected and best[0] / total >= thresh:
        return best[1]
    return None


def ratio_and_expected(seq, qual, lookup, count_of):
    """(best / total, expected errors) of a read, the two numbers the acceptance test compares; None where no candidate"""
    a = bytearray(seq)
    best, total = None, 0.0
    for pos in range(len(a)):
        qv = min(int(qual[pos]), BC_MAX_QV)
        existing = a[pos]
        for val in b"ACGT":
            if val == existing:
                continue
            a[pos] = val
            hit = lookup(bytes(a))
            if hit is not None:
                likelihood = probability(qv) * float(1 + count_of(hit))
                best = likelihood if best is None else max(best, likelihood)
                total += likelihood
        a[pos] = existing
    expected = 0.0
    for q in qual:
        expected += probability(int(q))
    return (None if best is None else best / total), expected


# ---- layout of a list ---------------------------------------------------------------------------------------------------
def ceil_log2(n):
    b = 0
    while (1 << b) < n:
        b += 1
    return b


class ListLayout:
    """the tables set_whitelist makes of a list's distinct raw keys: the pigeonhole bins of table A (by head) and table B (by
    tail) and the bins of the exact index"""

    def __init__(self, raw_keys, L):
        k = np.unique(np.asarray(raw_keys, U32)).astype(np.uint64)
        self.keys, self.L, self.m = k, L, len(k)
        hA = L // 2
        self.bitsA, self.bitsB = 2 * hA, 2 * (L - hA)
        self.head, self.tail = (k >> np.uint64(self.bitsB)).astype(np.int64), (k & np.uint64((1 << self.bitsB) - 1)).astype(np.int64)
        bitsE = ceil_log2(self.m) - 1 if ceil_log2(self.m) > 0 else 0
        bitsE = min(max(bitsE, self.bitsA), 2 * L, K["BITS_E_MAX"])
        self.bitsE, self.shiftE = bitsE, 2 * L - bitsE
        self.offA = np.concatenate([[0], np.cumsum(np.bincount(self.head, minlength=1 << self.bitsA))])
        self.offB = np.concatenate([[0], np.cumsum(np.bincount(self.tail, minlength=1 << self.bitsB))])
        self.offE = np.concatenate([[0], np.cumsum(np.bincount((k >> np.uint64(self.shiftE)).astype(np.int64), minlength=1 << bitsE))])

    def binE(self, key):
        b = int(key) >> self.shiftE
        return int(self.offE[b]), int(self.offE[b + 1])

    def binA(self, key):
        h = int(key) >> self.bitsB
        return int(self.offA[h]), int(self.offA[h + 1])

    def binB(self, key):
        t = int(key) & ((1 << self.bitsB) - 1)
        return int(self.offB[t]), int(self.offB[t + 1])


def cnt_shift_of(n_canon):
    s = 1
    while s < 32 and (1 << s) <= n_canon:
        s += 1
    return s


def hot_hash(keys):
    return ((np.asarray(keys, np.uint64) * np.uint64(K["HOT_MUL"])) & np.uint64(0xFFFFFFFF)) >> np.uint64(K["HOT_SHIFT"])


def hot_slots(key):
    b0 = int(hot_hash([key])[0])
    b1 = (b0 + 1) & (HOT_BUCKETS - 1)
    return [2 * b0, 2 * b0 + 1, 2 * b1, 2 * b1 + 1]


def first_of(n):
    """reads of the sampling batch of a call that builds a table"""
    f = min(n // K["FIRST_DIV"], K["FIRST_MAX"])
    return f // MB_TILE * MB_TILE


# ---- a case -------------------------------------------------------------------------------------------------------------
class Case:
    """libs: {library id: (raw keys, translate_to or None)}; canon: the canonical list, ascending, so that translate_to and a
    rank are the same number.  qualn: quality bytes, bit 7 = N.  prior: None (the VALID table after pass A) or the installed
    PRIOR table of library 0.  hot: the call is to build a table (the test sets CRGPU_HOT_MIN_READS=1)."""

    def __init__(self, name, L, canon, libs, cb, qualn, flags, max_expected=DBL_MAX, thresh=0.975, prior=None, hot=False, env=None):
        self.name, self.L = name, L
        self.canon = np.asarray(canon, U32)
        assert (np.diff(self.canon.astype(np.int64)) > 0).all()
        self.libs = {l: (np.asarray(k, U32), None if t is None else np.asarray(t, U32)) for l, (k, t) in libs.items()}
        self.cb, self.qualn, self.flags = np.ascontiguousarray(cb, U32), np.ascontiguousarray(qualn, np.uint8), np.ascontiguousarray(flags, np.uint8)
        self.n = len(self.cb)
        assert self.qualn.shape == (self.n, L) and self.flags.shape == (self.n,)
        assert np.array_equal((self.qualn & 0x80).any(axis=1), (self.flags & FLAG_HAS_N) != 0)   # the precondition of crgpu.h
        self.max_expected, self.thresh, self.prior, self.hot = max_expected, thresh, prior, hot
        self.env = dict(env or {})
        self.claims = []
        self._d = self._e = None

    def with_params(self, max_expected, thresh):
        c = Case(self.name, self.L, self.canon, self.libs, self.cb, self.qualn, self.flags, max_expected, thresh, self.prior, self.hot, self.env)
        c.claims, c._d = self.claims, self._d
        return c

    def ascii(self):
        s = unpack(self.cb, self.L)
        s[(self.qualn & 0x80) != 0] = ord("N")
        return s, self.qualn & 0x7F

    def rank_tables(self, lib):
        """(distinct raw keys ascending, the rank of each): HashMap::collect keeps the LAST duplicate (whitelist.rs:301-311)"""
        keys, tr = self.libs[lib]
        rank = np.searchsorted(self.canon, keys).astype(np.int64) if tr is None else tr.astype(np.int64)
        if tr is None:
            assert (self.canon[np.minimum(rank, len(self.canon) - 1)] == keys).all()
        order = np.argsort(keys, kind="stable")
        ks, rs = keys[order], rank[order]
        last = np.concatenate([ks[1:] != ks[:-1], [True]])
        return ks[last], rs[last]


class Expected:
    pass


def expected(case, no_qual=False):
    """idx after pass A and pass B, the corrected bytes and both histograms of every configured library, from
    correct_barcode().  no_qual: the host entry points without qualities (qual = None; an N is still an N)."""
    if case._e is not None and not no_qual:
        return case._e
    e = Expected()
    n, L = case.n, case.L
    lib = (case.flags & FLAG_LIB_MASK).astype(np.int64)
    has_n = (case.flags & FLAG_HAS_N) != 0
    e.idx_a = np.full(n, MISS, U32)
    tables = {}
    for l in case.libs:
        ks, rs = case.rank_tables(l)
        tables[l] = (ks, rs)
        sel = (lib == l) & ~has_n
        pos = np.minimum(np.searchsorted(ks, case.cb[sel]), len(ks) - 1)
        hit = ks[pos] == case.cb[sel]
        e.idx_a[np.nonzero(sel)[0][hit]] = rs[pos[hit]].astype(U32)
    nc = len(case.canon)
    e.valid = {l: np.bincount(e.idx_a[(lib == l) & (e.idx_a != MISS)].astype(np.int64), minlength=nc).astype(U32) for l in case.libs}
    e.idx_b = e.idx_a.copy()
    e.corrected = np.zeros(n, np.uint8)
    seqs, quals = case.ascii()
    todo = np.nonzero((e.idx_a == MISS) & np.isin(lib, list(case.libs)))[0]
    memo = {}
    for l in case.libs:
        ks, rs = tables[l]
        mine = todo[lib[todo] == l]
        if not len(mine):
            continue
        # every key one substitution from a miss (an N read: the four completions are among the neighbours of its packed key
        # or that key itself), looked up once: the dictionary the restatement's membership test reads
        ck = np.unique(case.cb[mine].astype(np.uint64))
        cand = [ck]
        for p in range(L):
            for b in range(4):
                sh = np.uint64(2 * p)
                cand.append((ck & ~(np.uint64(3) << sh)) | (np.uint64(b) << sh))
        cand = np.unique(np.concatenate(cand)).astype(U32)
        pos = np.minimum(np.searchsorted(ks, cand), len(ks) - 1)
        ok = ks[pos] == cand
        member = dict(zip(cand[ok].tolist(), rs[pos[ok]].tolist()))
        prior = case.prior if (case.prior is not None and l == 0) else e.valid[l]
        canon_seq = {}

        def lookup(s, member=member, canon_seq=canon_seq):
            if b"N" in s:
                return None
            r = member.get(key_of(s))
            if r is None:
                return None
            if r not in canon_seq:
                canon_seq[r] = seq_of(int(case.canon[r]), L)
            return canon_seq[r]

        def count_of(s, prior=prior):
            return int(prior[int(np.searchsorted(case.canon, U32(key_of(s))))])
        for i in mine:
            q = None if no_qual else bytes(quals[i])
            tag = (l, seqs[i].tobytes(), q)
            if tag not in memo:
                out = correct_barcode(seqs[i].tobytes(), q, lookup, count_of, case.max_expected, case.thresh)
                memo[tag] = MISS if out is None else int(np.searchsorted(case.canon, U32(key_of(out))))
            if memo[tag] != MISS:
                e.idx_b[i] = memo[tag]
                e.corrected[i] = 1
    e.corrected_hist = {l: np.bincount(e.idx_b[(lib == l) & (e.corrected == 1)].astype(np.int64), minlength=nc).astype(U32) for l in case.libs}
    if not no_qual:
        case._e = e
    return e


def read_numbers(case, i):
    """(best / total, expected errors) of read i of a one-library case, by the restatement"""
    ks, rs = case.rank_tables(0)
    member = dict(zip(ks.tolist(), rs.tolist()))
    prior = case.prior if case.prior is not None else expected(case).valid[0]

    def lookup(s):
        if b"N" in s:
            return None
        r = member.get(key_of(s))
        return None if r is None else seq_of(int(case.canon[r]), case.L)
    seqs, quals = case.ascii()
    return ratio_and_expected(seqs[i].tobytes(), bytes(quals[i]), lookup, lambda s: int(prior[int(np.searchsorted(case.canon, U32(key_of(s))))]))


# ---- the structure of a case, recomputed --------------------------------------------------------------------------------
class Described:
    pass


def describe(case):
    """where pass A and pass B put every read of the case: from the arrays and the restated layout alone"""
    if case._d is not None:
        return case._d
    d = Described()
    e = expected(case)
    n = case.n
    d.n, d.n_canon = n, len(case.canon)
    d.buckets_per_lib = (d.n_canon + BIN_SIZE - 1) // BIN_SIZE
    d.cnt_shift = cnt_shift_of(d.n_canon)
    d.lists = {l: ListLayout(k, case.L) for l, (k, _) in case.libs.items()}
    d.miss = e.idx_a == MISS
    d.first = first_of(n) if (case.hot and n >= N_TABLE and len(case.libs) == 1) else 0
    d.table = d.first > 0
    if d.table:
        m = n - d.first
        grid = min((m + MB_TILE - 1) // MB_TILE, 256)
        r = np.arange(m)                                    # one round: workgroup g takes the chunks g, g + grid, ...
        d.chunk = r // LH_CHUNK
        tid = r % LH_THREADS
        d.wave = tid // 64
        d.region = d.chunk % grid * LH_WAVES + d.wave
        d.order = (d.chunk // grid * LH_ITEMS + (r % LH_CHUNK) // LH_THREADS) * 64 + tid % 64      # records: by item, then lane
        miss = d.miss[d.first:]
        rec = np.nonzero(miss)[0]
        rec = rec[np.lexsort((d.order[rec], d.region[rec]))]        # the records, region after region
        d.rec_reads = rec + d.first
        d.rec_count = np.bincount(d.region[miss], minlength=REGIONS)
        # barcode order: a stable sort of the records on the key bits
        d.sorted_reads = d.rec_reads[np.argsort(case.cb[d.rec_reads], kind="stable")]
        fl = case.flags[d.sorted_reads]
        d.sorted_keys = case.cb[d.sorted_reads]
        d.sorted_usable = ((fl & FLAG_HAS_N) == 0) & ((fl & FLAG_LIB_MASK) == min(case.libs))
        # counted table rounds
        d.counted = n >= N_COUNTED_MIN      # (unless CRGPU_K1_SPLIT=0 stages every round in full)
        samp = case.cb[:d.first][~d.miss[:d.first]]
        d.sampled = np.unique(samp)
    case._d = d
    return d


def sorted_chunks(d):
    """per 64-record chunk of the sorted records: the runs of equal keys as (first lane, length, usable lanes)"""
    out = []
    for c0 in range(0, len(d.sorted_keys), 64):
        k, u = d.sorted_keys[c0:c0 + 64], d.sorted_usable[c0:c0 + 64]
        heads = np.nonzero(np.concatenate([[True], k[1:] != k[:-1]]))[0]
        ends = np.concatenate([heads[1:], [len(k)]])
        out.append([(int(a), int(b - a), int(u[a:b].sum()), bool(u[a])) for a, b in zip(heads, ends)])
    return out


# ---- building blocks ----------------------------------------------------------------------------------------------------
Q0 = 60   # the quality of a base nothing is said about (phred 27)


def spread_list(n):
    """n distinct ascending 16-base keys, evenly spread over the 32-bit space"""
    step = min(((1 << 32) - 20000) // n, 4093)
    return (np.arange(n, dtype=np.uint64) * np.uint64(step) + np.uint64(12345)).astype(U32)


def far_centers(k, L, rng, min_dist=6, avoid=()):
    """k keys of L bases at pairwise Hamming distance >= min_dist (clusters built around them do not touch)"""
    out = list(avoid)
    while len(out) < k + len(avoid):
        c = int(rng.integers(0, 1 << (2 * L)))
        if all(hamming(c, o, L) >= min_dist for o in out):
            out.append(c)
    return out[len(avoid):]


class Reads:
    """reads of one call, filled with exact hits; put() overwrites single reads"""

    def __init__(self, n, L, fill_keys, rng, lib=0):
        self.n, self.L = n, L
        self.cb = np.asarray(fill_keys, U32)[rng.integers(0, len(fill_keys), n)]
        self.qualn = np.full((n, L), Q0, np.uint8)
        self.flags = np.full(n, lib, np.uint8)

    def put(self, i, key, qual=None, n_at=(), lib=None):
        self.cb[i] = key
        self.qualn[i] = Q0 if qual is None else qual
        for p in n_at:
            assert get_base(int(key), self.L, p) == 0     # N packs as A
            self.qualn[i, p] |= 0x80
        self.flags[i] = (self.flags[i] & FLAG_LIB_MASK if lib is None else lib) | (FLAG_HAS_N if len(n_at) else 0)
        return i


def candidates(case, i, lib=0):
    """(slot = position * 4 + base, rank) of the listed barcodes one substitution from read i, as the reference visits them"""
    ks, rs = case.rank_tables(lib)
    member = dict(zip(ks.tolist(), rs.tolist()))
    key, L = int(case.cb[i]), case.L
    n_at = np.nonzero(case.qualn[i] & 0x80)[0]
    out = []
    if len(n_at) > 1:
        return out
    for p in (range(L) if not len(n_at) else [int(n_at[0])]):
        for b in range(4):
            if not len(n_at) and b == get_base(key, L, p):
                continue
            r = member.get(set_base(key, L, p, b))
            if r is not None:
                out.append((p * 4 + b, int(r)))
    return out


# ---- group E: the decision ----------------------------------------------------------------------------------------------
def decision_case(translated=False):
    """Clusters of listed barcodes around far-apart centres; the reads are the centres (not listed) with chosen qualities and
    Ns, all behind the sampling batch, and once more inside it.  A PRIOR table is installed.  translated: the list's ranks
    run against its raw order (key at sorted position p translates to canon[m - 1 - p])."""
    L, n = 16, N_TABLE
    rng = np.random.default_rng(7)
    C = far_centers(14, L, rng)
    wl, prior_of, reads, tags = [], {}, [], {}

    def other(key, pos, k=1):
        return set_base(key, L, pos, (get_base(key, L, pos) + k) & 3)

    def add(key, prior=0):
        wl.append(key)
        prior_of[key] = prior
        return key

    def read(tag, key, qual=None, n_at=()):
        tags[tag] = len(reads)
        reads.append((key, qual, n_at))

    def q_at(**kw):
        q = np.full(L, Q0, np.uint8)
        for k, v in kw.items():
            q[int(k[1:])] = v
        return q
    # two candidates of equal likelihood: best / total is 0.5 exactly.  The candidate at position 3 is met first; in tie2 it is
    # the smaller sequence (the larger one comes second), in tie2_rev the larger one
    c0 = set_base(C[0], L, 3, 2)
    add(set_base(c0, L, 3, 0), 5), add(other(c0, 12), 5)
    read("tie2", c0)
    c13 = set_base(C[13], L, 3, 1)
    add(set_base(c13, L, 3, 3), 5), add(other(c13, 12), 5)
    read("tie2_rev", c13)
    # three candidates, different priors: its ratio is used as the threshold
    add(other(C[1], 1), 3), add(other(C[1], 6), 9), add(other(C[1], 14), 4)
    read("ratio3", C[1], q_at(p1=50, p6=58, p14=44))
    # the quality cap: 66, 67 and 127 at the mutated position weigh the same, 65 weighs more; the expected-error sum is uncapped
    add(other(C[2], 5), 2), add(other(C[2], 9), 2)
    for q in (65, 66, 67, 127):
        read("cap%d" % q, C[2], q_at(p5=q, p9=66))
    # priors 0, 1 and 2^32 - 1
    add(other(C[3], 2), 0), add(other(C[3], 7), 1), add(other(C[3], 13), 0xFFFFFFFF)
    read("prior_max", C[3])
    add(other(C[4], 2), 0), add(other(C[4], 7), 1)
    read("prior01", C[4])
    # one N: four completions at position 0, one at the last position, none (a neighbour elsewhere does not count), four at the
    # last position; two Ns
    c5 = set_base(C[5], L, 0, 0)
    for b in range(4):
        add(set_base(c5, L, 0, b), 9 if b == 3 else 0)
    read("n4_first", c5, n_at=(0,))
    c5b = set_base(c5, L, 5, 0)
    add(set_base(set_base(c5b, L, 0, 1), L, 5, 2))
    read("n_two", c5b, n_at=(0, 5))
    c6 = set_base(C[6], L, L - 1, 0)
    add(set_base(c6, L, L - 1, 2), 1)
    read("n1_last", c6, n_at=(L - 1,))
    c7 = set_base(C[7], L, 0, 0)
    add(other(c7, 4), 1)
    read("n0_first", c7, n_at=(0,))
    c8 = set_base(C[8], L, L - 1, 0)
    for b in range(4):
        add(set_base(c8, L, L - 1, b), 3 - b)
    read("n4_last", c8, q_at(p15=40), n_at=(L - 1,))
    # an N read and a read with a real A there pack to the same key
    c9 = set_base(C[9], L, 3, 0)
    add(set_base(c9, L, 3, 1), 1), add(other(c9, 10), 6)
    read("same_key_a", c9)
    read("same_key_n", c9, n_at=(3,))
    # all 48 neighbours listed: candidates in slots 0 and 63
    c10 = set_base(set_base(C[10], L, 0, 2), L, L - 1, 1)
    for j, k in enumerate(neighbours(c10, L)):
        add(k, j % 5)
    read("all48", c10)
    read("all48_q", c10, np.array([40 + 3 * (p % 9) for p in range(L)], np.uint8))
    # one candidate: the shortcut that does not read the qualities
    add(other(C[11], 8), 4)
    read("lone", C[11])
    read("lone_q34", C[11], q_at(p8=34))
    # a near tie against different priors: q 50 x (1 + 9) against q 60 x (1 + 99)
    add(other(C[12], 4), 9), add(other(C[12], 11), 99)
    read("tie_q_prior", C[12], q_at(p4=50, p11=60))
    # filler: listed barcodes nobody is near
    fill = far_centers(64, L, rng, avoid=C + wl)
    for k in fill:
        add(k, 1)
    wl = np.array(sorted(set(wl)), U32)
    assert len(wl) == len(prior_of)
    m = len(wl)
    tr = (m - 1 - np.arange(m)).astype(U32) if translated else None
    rk = Reads(n, L, np.array(fill, U32), rng)
    first = first_of(n)
    at = {}
    for tag, j in tags.items():
        key, qual, n_at = reads[j]
        at[tag] = rk.put(first + 100 + 67 * j, key, qual, n_at)       # spread over the waves of the first chunk
        rk.put(10 + j, key, qual, n_at)                              # the same read in the sampling batch: scanned
    prior = np.zeros(m, U32)
    for k, v in prior_of.items():
        p = int(np.searchsorted(wl, k))
        prior[int(tr[p]) if translated else p] = v
    case = Case("decision_translated" if translated else "decision", L, wl, {0: (wl, tr)}, rk.cb, rk.qualn, rk.flags, prior=prior, hot=True)
    case.at = at
    cl = case.claims
    cl.append(dict(kind="behind_first", reads=sorted(at.values())))
    cl.append(dict(kind="ratio", read=at["tie2"], value=0.5, n_cand=2))
    cl.append(dict(kind="ratio", read=at["tie2_rev"], value=0.5, n_cand=2))
    cl.append(dict(kind="tie_orders", reads=[at["tie2"], at["tie2_rev"]]))
    cl.append(dict(kind="n_cand", read=at["tie_q_prior"], count=2))      # (equal on paper; in doubles the two may differ by an ulp)
    cl.append(dict(kind="n_cand", read=at["ratio3"], count=3))
    for q in (66, 67, 127):
        cl.append(dict(kind="ratio", read=at["cap%d" % q], value=0.5, n_cand=2))
    cl.append(dict(kind="ratio_above", read=at["cap65"], value=0.5))
    cl.append(dict(kind="expected_order", reads=[at["cap127"], at["cap67"], at["cap66"], at["cap65"]]))
    cl.append(dict(kind="priors", read=at["prior_max"], values=[0, 1, 0xFFFFFFFF]))
    cl.append(dict(kind="priors", read=at["prior01"], values=[0, 1]))
    for tag, cnt, slots in (("n4_first", 4, [0, 1, 2, 3]), ("n1_last", 1, [4 * (L - 1) + 2]), ("n0_first", 0, []), ("n4_last", 4, [60, 61, 62, 63]),
                            ("n_two", 0, []), ("same_key_n", 1, [13]), ("same_key_a", 2, None), ("all48", 48, None), ("lone", 1, None)):
        cl.append(dict(kind="n_cand", read=at[tag], count=cnt, slots=slots))
    cl.append(dict(kind="has_slots", read=at["all48"], slots=[0, 63]))
    cl.append(dict(kind="same_key", reads=[at["same_key_a"], at["same_key_n"]]))
    if translated:
        cl.append(dict(kind="larger_rank_is_smaller_raw", read=at["tie2"]))
    return case


def decision_params(case):
    """(name, max_expected, thresh) of the runs of group E: the equalities come from the restatement's own numbers"""
    r3, _ = read_numbers(case, case.at["ratio3"])
    _, s67 = read_numbers(case, case.at["cap67"])
    inf = float("inf")
    return [("tie_at_half", DBL_MAX, 0.5), ("tie_above_half", DBL_MAX, math.nextafter(0.5, 1.0)),
            ("ratio_equal", DBL_MAX, r3), ("ratio_above", DBL_MAX, math.nextafter(r3, 1.0)),
            ("veto_equal", s67, 0.5), ("veto_above", math.nextafter(s67, inf), 0.5),
            ("thresh_one", DBL_MAX, 1.0), ("thresh_above_one", DBL_MAX, math.nextafter(1.0, 2.0)), ("thresh_nan", DBL_MAX, float("nan")),
            ("max_expected_zero", 0.0, 0.5), ("max_expected_negative", -1.0, 0.5), ("veto_on_lone", 5.0, 0.975)]


# ---- group F: barcode order ---------------------------------------------------------------------------------------------
F_T0 = key_of("ACGTACGT")     # the tail of every miss of family A
F_TF = key_of("TTTTGGGG")     # the tail of the fillers: no listed barcode has it or a neighbour of it
F_HB = 0xFFF0                 # the head of the misses of family B (found through table B)
F_BINS = (1, 7, 8, 9)


def _two_off(t, nbits):
    """16-bit halves two substitutions from t, ascending (never a candidate of t)"""
    L = nbits // 2
    out = set()
    for p in range(L):
        for q in range(p + 1, L):
            for a in (1, 2, 3):
                for b in (1, 2, 3):
                    out.add(t ^ (a << (2 * p)) ^ (b << (2 * q)))
    return sorted(out)


def sorted_case(name="sorted"):
    """Runs of equal keys placed on chosen lanes of the sorted records (k_correct_sorted).  A miss of family A is (head, F_T0):
    its candidates are the entries of the head's bin of table A whose tail is one substitution from F_T0; a filler is
    (head, F_TF) with an empty bin; family B mirrors A through table B.  The heads ascend with the run number, so the sorted
    order is the order of the runs below."""
    L, n = 16, N_TABLE
    rng = np.random.default_rng(11)
    first = first_of(n)
    wl, runs = [], []        # runs: dict(key, reads=[(qual, kind)], ...) in sorted order
    far2 = _two_off(F_T0, 16)
    state = dict(head=8, nb=0)

    def bin_for(head, size, cand_tails, cand_last):
        """list `size` tails under `head`: the candidate tails and tails two substitutions from F_T0 on one side of them"""
        others = [t for t in far2 if (t > max(cand_tails) if not cand_last else t < min(cand_tails))]
        assert len(others) >= size - len(cand_tails)
        for t in list(cand_tails) + others[:size - len(cand_tails)]:
            wl.append((head << 16) | t)

    def run(length, cand=True, kinds=None, quals=None, two=False, size=None):
        """a run of `length` equal keys; kinds: per read 'ok', 'lib' (another library) or 'n' (an N at position 0)"""
        head = state["head"]
        state["head"] += 1
        if kinds and "n" in kinds:
            head &= 0x3FFF     # (position 0 is an A)
        r = dict(key=(head << 16) | (F_T0 if cand else F_TF), length=length, cand=cand, kinds=kinds or ["ok"] * length, quals=quals, two=two)
        if cand:
            size = F_BINS[state["nb"] % 4] if size is None else size
            last = (state["nb"] // 4) % 2 == 1
            state["nb"] += 1
            tails = [F_T0 ^ 1] + ([F_T0 ^ (2 << 14)] if two else [])     # last base (position 15) / first base of the tail (position 8)
            bin_for(head, max(size, len(tails)), tails, last)
            r["size"] = max(size, len(tails))
        runs.append(r)
        return r

    def lane():
        return sum(r["length"] for r in runs) % 64

    def pad_to(l, singles=False):
        while lane() != l:
            run(1 if singles else (l - lane()) % 64, cand=False)
    marks = {}

    def mark(tag):
        marks[tag] = sum(r["length"] for r in runs)
    wl.append((4 << 16) | 0x0001)                 # one entry below everything: the bins that follow start at odd offsets
    mark("c_singles")
    run(1)                                        # chunk 0: 64 runs of one read, the first and the last with candidates
    while lane() != 63:
        run(1, cand=lane() % 9 == 4)
    mark("r63_at63"), run(63)                     # 63 equal keys from lane 63
    pad_to(63)
    mark("r64_at63"), run(64)
    pad_to(63)
    mark("r65_at63"), run(65)
    pad_to(0)
    while (sum(r["length"] for r in runs) // 64) % KS_WAVES != KS_WAVES - 3:     # the run of 64 below: one chunk before a workgroup's last
        run(64, cand=False)
    mark("r63_at0"), run(63), run(1)
    mark("r64_at0"), run(64)
    mark("r65_at0"), run(65)
    pad_to(0)
    mark("c_heads"), [run(8) for _ in range(KS_HEADS)]                       # exactly KS_HEADS runs in a chunk
    assert lane() == 0
    mark("c_heads1"), [run(7) for _ in range(KS_HEADS)], run(64 - 7 * KS_HEADS)   # KS_HEADS + 1: the last run is a batch of its own
    assert lane() == 0
    mark("r_lib_head"), run(6, kinds=["lib"] + ["ok"] * 5)                    # headed by a record without an index
    mark("r_n_head"), run(6, kinds=["n"] + ["ok"] * 5)
    mark("r_all_lib"), run(4, kinds=["lib"] * 4)
    pad_to(0)
    mark("c_indexless"), [run(4, kinds=["lib"] * 4) for _ in range(KS_HEADS)]   # a whole batch without a usable lane ...
    run(8), run(8)                                                            # ... and a batch behind it that has some
    pad_to(0)
    # reads of one run that disagree on the winner: two candidates (positions 8 and 15), the qualities decide
    qa, qb = np.full(L, Q0, np.uint8), np.full(L, Q0, np.uint8)
    qa[8], qb[15] = 40, 40
    mark("r_disagree"), run(6, quals=[qa, qa, qb, qb, qb, qa], two=True)
    run(5, two=True)                                                          # (and one that agrees, with two candidates)
    pad_to(0)
    # a second even start for every bin size: one more single entry flips the parity of what follows
    wl.append((state["head"] << 16) | 0x0002)
    state["head"] += 1
    mark("c_parity"), [run(2) for _ in range(8)]
    run(3, size=20)
    mark("end_a")
    # family B: the same through table B -- misses (F_HB, tail), listed (a head one or two substitutions from F_HB, tail)
    farh = _two_off(F_HB, 16)
    tails_b = [t for t in range(0x4000, 0x4000 + 64) if hamming(t, F_T0, 8) > 2 and hamming(t, F_TF, 8) > 2]
    wl.append((5 << 16) | (tails_b[0] - 1))       # parity of table B below the first bin
    nb = 0
    for rep in range(2):
        for size in F_BINS:
            t = tails_b[nb]
            nb += 1
            cand_head = F_HB ^ 1
            others = [h for h in farh if (h < cand_head if rep else h > cand_head)][:size - 1]
            for h in [cand_head] + others:
                wl.append((h << 16) | t)
            runs.append(dict(key=(F_HB << 16) | t, length=3, cand=True, kinds=["ok"] * 3, quals=None, two=False, size=size, table="B"))
        # (1 + 7 + 8 + 9 entries: the second repetition starts at the other parity)
    mark("end")
    fill = [((0x2000 + j) << 16) | 0x3C3C for j in range(200)]      # the barcodes of the reads that hit: nobody's candidates
    wl = np.array(sorted(set(wl + fill)), U32)
    rk = Reads(n, L, fill, rng)
    i = first + 64
    for r in runs:
        if any(k != "ok" for k in r["kinds"]):
            i = (i + 63) // 64 * 64 if (i % 64) + r["length"] > 64 else i     # inside one 64-read block: record order = read order
        for j in range(r["length"]):
            kind = r["kinds"][j]
            rk.put(i, r["key"], None if r["quals"] is None else r["quals"][j], n_at=(0,) if kind == "n" else (), lib=1 if kind == "lib" else None)
            i += 1
    assert i <= n
    case = Case(name, L, wl, {0: (wl, None)}, rk.cb, rk.qualn, rk.flags, hot=True, env={"CRGPU_K2_SORTED": "1"})
    case.marks = marks
    cl = case.claims
    cl.append(dict(kind="sorted_total", total=marks["end"]))
    cl.append(dict(kind="chunk_runs", chunk=marks["c_singles"] // 64, runs=64))
    for tag, length, at in (("r63_at63", 63, 63), ("r64_at63", 64, 63), ("r65_at63", 65, 63), ("r63_at0", 63, 0), ("r64_at0", 64, 0), ("r65_at0", 65, 0)):
        cl.append(dict(kind="run", pos=marks[tag], length=length, lane=at))
    cl.append(dict(kind="run_in_wave", pos=marks["r64_at0"], wave=KS_WAVES - 2))
    cl.append(dict(kind="chunk_runs", chunk=marks["c_heads"] // 64, runs=KS_HEADS, wanted=KS_HEADS))
    cl.append(dict(kind="chunk_runs", chunk=marks["c_heads1"] // 64, runs=KS_HEADS + 1, wanted=KS_HEADS + 1))
    cl.append(dict(kind="indexless_head", pos=marks["r_lib_head"], usable=5))
    cl.append(dict(kind="indexless_head", pos=marks["r_n_head"], usable=5))
    cl.append(dict(kind="indexless_batch", chunk=marks["c_indexless"] // 64))
    cl.append(dict(kind="run_disagrees", pos=marks["r_disagree"], pattern=[0, 0, 1, 1, 1, 0]))
    cl.append(dict(kind="bins", table="A", sizes=[0, 1, 7, 8, 9], also=20))
    cl.append(dict(kind="bins", table="B", sizes=[0, 1, 7, 8, 9]))
    return case


def sorted_total_case(total):
    """`total` recorded misses, every one with a candidate, on distinct keys"""
    L, n = 16, N_TABLE
    rng = np.random.default_rng(13)
    wl = spread_list(4096)
    rk = Reads(n, L, wl, rng)
    first = first_of(n)
    for j in range(total):
        rk.put(first + 17 + 131 * j, int(wl[5 + 7 * j]) ^ 1)
    case = Case("sorted_total_%d" % total, L, wl, {0: (wl, None)}, rk.cb, rk.qualn, rk.flags, hot=True, env={"CRGPU_K2_SORTED": "1"})
    case.claims.append(dict(kind="sorted_total", total=total))
    case.claims.append(dict(kind="all_corrected", count=total))
    return case


def dense8_case():
    """8-base barcodes on a list of four fifths of all of them: a bin of either table holds ~205 entries, so the eight runs of a
    wave bring more than 64 search items (a second round of the item loop), and ties between candidates abound"""
    L, n = 8, N_TABLE
    rng = np.random.default_rng(17)
    allk = np.arange(1 << 16, dtype=U32)
    wl = allk[(allk * 7 + (allk >> 8)) % 5 != 0]
    out = allk[(allk * 7 + (allk >> 8)) % 5 == 0]
    rk = Reads(n, L, wl, rng)
    first = first_of(n)
    pick = out[rng.choice(len(out), 40, replace=False)]
    i = first + 5
    for j, k in enumerate(sorted(pick.tolist())):
        for t in range(8):
            q = np.full(L, Q0, np.uint8)
            q[(j + t) % L] = 40 + t
            rk.put(i, k, q if t % 2 else None)
            i += 1
    case = Case("dense8", L, wl, {0: (wl, None)}, rk.cb, rk.qualn, rk.flags, thresh=0.02, hot=True, env={"CRGPU_K2_SORTED": "1"})
    case.claims.append(dict(kind="sorted_total", total=320))
    case.claims.append(dict(kind="all_corrected", count=320))
    case.claims.append(dict(kind="chunk_runs", chunk=0, runs=8, wanted=8))
    case.claims.append(dict(kind="items_in_batch", chunk=0, more_than=64))
    return case


# ---- group G: the records in record order -------------------------------------------------------------------------------
def records_case(n_list, name):
    """Regions (waves of the lookup's first workgroup) with 1, 3, 4, 5, 256 and 257 records; N reads that fill the queue of one
    wave of k_correct_records to 63 and to exactly 64; regions that mix N reads and plain misses; misses inside the sampling
    batch with the keys of recorded ones.  n_list: at most 31 x 32768 barcodes (staged CORRECTED histogram) or more."""
    L, n = 16, N_TABLE
    rng = np.random.default_rng(19)
    wl = spread_list(n_list)
    rk = Reads(n, L, wl, rng)
    first = first_of(n)
    sel = wl[(wl & 3) != 1][:: max(1, len(wl) // 3000)]             # barcodes whose last base can become a C that is not theirs
    plain = (sel & ~U32(3)) | U32(1)
    ok = ~np.isin(plain, wl)
    plain = plain[ok]
    na = wl[((wl >> 30) & 3) == 0][:: max(1, len(wl) // 3000)]      # barcodes that start with an A: an N at position 0 has a completion

    def slot(wave, k):
        """the k-th read of wave `wave` of the first chunk, in record order"""
        return first + (k // 64) * LH_THREADS + wave * 64 + k % 64
    counts = {0: 1, 1: 3, 2: 4, 3: 5, 4: 257, 5: 256, 6: 256, 7: 40}
    j = 0
    for wave, cnt in counts.items():
        for k in range(cnt):
            as_n = (wave == 5 and k < 63) or (wave == 6 and k < 64) or (wave in (4, 7) and k % 3 == 0)
            if as_n:
                rk.put(slot(wave, k), int(na[j % len(na)]), n_at=(0,))
            else:
                rk.put(slot(wave, k), int(plain[j % len(plain)]))
            j += 1
    for k in range(50):      # the same keys before `first`: scanned, not recorded
        rk.put(20 + k, int(plain[k]))
        rk.put(200 + k, int(na[k]), n_at=(0,))
    case = Case(name, L, wl, {0: (wl, None)}, rk.cb, rk.qualn, rk.flags, hot=True, env={"CRGPU_K2_SORTED": "0"})
    case.claims.append(dict(kind="region_counts", counts=counts))
    case.claims.append(dict(kind="n_queue", region=5, part=0, wave=0, peak=63))
    case.claims.append(dict(kind="n_queue", region=6, part=0, wave=0, peak=64))
    case.claims.append(dict(kind="empty_parts", region=0, empty=K2_PARTS - 1))
    case.claims.append(dict(kind="buckets", staged=n_list <= SI_MISS_BUCKET * BIN_SIZE))
    case.claims.append(dict(kind="sampled_misses_share_keys", at_least=40))
    return case


def records_big_case():
    """The smallest call in which a workgroup of the lookup takes three chunks, so that one wave's region holds 1536 records and a
    part of it more than 256: a wave of k_correct_records then queues N reads in two steps -- 1 + 64 = 65 in one part (the last 64
    are drained, the first stays), 63 + 64 = 127 in another."""
    L = 16
    m = (2 * 256 + 1) * LH_CHUNK
    n = m * 4 // 3
    assert first_of(n) == n - m
    rng = np.random.default_rng(43)
    wl = spread_list(200_000)
    rk = Reads(n, L, wl, rng)
    first = first_of(n)
    plain = (wl[::40] & ~U32(3)) | ((wl[::40] + U32(1)) & U32(3))
    plain = plain[~np.isin(plain, wl)]
    na = wl[((wl >> 30) & 3) == 0][::10]
    per = LH_ITEMS * 64                  # records of region 0 per chunk

    def slot(k):
        """the k-th record of region 0 (wave 0 of workgroup 0: chunks 0, 256, 512)"""
        c, k = divmod(k, per)
        return first + c * 256 * LH_CHUNK + (k // 64) * LH_THREADS + k % 64
    part = 3 * per // K2_PARTS           # 384 records
    n_at = set([5] + list(range(256, 320)) + list(range(part, part + 63)) + list(range(part + 256, part + 320)) + list(range(2 * part, 3 * per, 7)))
    for k in range(3 * per):
        if k in n_at:
            rk.put(slot(k), int(na[k % len(na)]), n_at=(0,))
        else:
            rk.put(slot(k), int(plain[k % len(plain)]))
    case = Case("records_big", L, wl, {0: (wl, None)}, rk.cb, rk.qualn, rk.flags, hot=True, env={"CRGPU_K2_SORTED": "0"})
    case.claims.append(dict(kind="region_counts", counts={0: 3 * per}))
    case.claims.append(dict(kind="n_queue", region=0, part=0, wave=0, peak=65))
    case.claims.append(dict(kind="n_queue", region=0, part=1, wave=0, peak=127))
    return case


# ---- group D: exactly full regions --------------------------------------------------------------------------------------
def record_cap_case(cap, surplus):
    """wave 3 of the first workgroup holds cap + surplus misses, every other wave fewer than cap"""
    L, n = 16, N_TABLE
    rng = np.random.default_rng(23)
    wl = spread_list(5000)
    rk = Reads(n, L, wl, rng)
    first = first_of(n)
    miss = (wl[::5] & ~U32(3)) | ((wl[::5] + U32(1)) & U32(3))
    miss = miss[~np.isin(miss, wl)]
    j = 0
    for wave in range(LH_WAVES):
        for k in range(cap + surplus if wave == 3 else (wave % cap)):
            rk.put(first + (k % LH_ITEMS) * LH_THREADS + wave * 64 + 7 * k % 64, int(miss[j]))
            j += 1
    for k in range(9):
        rk.put(first + LH_CHUNK + 70 * k, int(miss[j + k]))        # the second workgroup's waves: one miss each at most
    case = Case("record_cap_%d_plus_%d" % (cap, surplus), L, wl, {0: (wl, None)}, rk.cb, rk.qualn, rk.flags, hot=True,
                env={"CRGPU_MISS_RECORD_CAP": str(cap)})
    case.claims.append(dict(kind="fullest_region", region=3, count=cap + surplus, others_below=cap))
    return case


# ---- group C: the table of frequent barcodes ----------------------------------------------------------------------------
def table_case(k, full, cold_cap=None, cold_surplus=0):
    """A list of 2^k - 1 (or, full, 2^k) barcodes and the smallest call whose table rounds are counted.  The top rank is the
    most frequent barcode.  Barcode X collects, in one chunk each (one workgroup each), exactly cnt_max, cnt_max + 1 and
    cnt_max + 2 hits, two whole fields, and two fields and one.  Five barcodes with one hot_hash: four find a slot, one does
    not and is counted through the cold path.  cold_cap: one wave holds exactly cold_cap + cold_surplus cold hits."""
    L, n = 16, N_COUNTED
    rng = np.random.default_rng(29 + k)
    n_list = (1 << k) - (0 if full else 1)
    wl = spread_list(n_list)
    shift = cnt_shift_of(n_list)
    cnt_max = 0xFFFFFFFF >> shift
    first = first_of(n)
    top = int(wl[-1])
    h = hot_hash(wl).astype(np.int64)
    by = np.argsort(h, kind="stable")
    hs = h[by]
    # a crowd of five barcodes on one hash value, and X alone in its two buckets
    start = np.nonzero(np.concatenate([[True], hs[1:] != hs[:-1]]))[0]
    size = np.diff(np.concatenate([start, [len(hs)]]))
    g = int(start[np.nonzero(size >= 5)[0][3]])
    crowd = [int(x) for x in wl[by[g:g + 5]]]
    hc = int(hs[g])
    taken = {hc, (hc + 1) % HOT_BUCKETS, (hc - 1) % HOT_BUCKETS, int(hot_hash([top])[0]), (int(hot_hash([top])[0]) + 1) % HOT_BUCKETS,
             (int(hot_hash([top])[0]) - 1) % HOT_BUCKETS}
    X = next(int(x) for x, hx in zip(wl[1000:], h[1000:]) if all(((int(hx) + d) % HOT_BUCKETS) not in taken for d in (-1, 0, 1)))
    cb = np.full(n, top, U32)
    qualn = np.full((n, L), Q0, np.uint8)
    flags = np.zeros(n, np.uint8)
    cb[100:100 + 40] = X
    for j, c in enumerate(crowd):
        cb[300 + 10 * j:300 + 10 * j + 5 + j] = c
    x_hits = [cnt_max, cnt_max + 1, cnt_max + 2, 2 * (cnt_max + 1), 2 * (cnt_max + 1) + 1]
    x_hits = [x for x in x_hits if x <= LH_CHUNK]
    for c, cnt in enumerate(x_hits):
        at = first + c * LH_CHUNK + rng.permutation(LH_CHUNK)[:cnt]
        cb[at] = X
    base = first + len(x_hits) * LH_CHUNK
    # cold hits: barcodes the sampling batch has not seen, two in every wave of the chunks that follow; the crowd's reads
    cold = wl[5000:5000 + 4000]
    cold = cold[~np.isin(cold, crowd + [X, top])]
    n_chunks = (n - base) // LH_CHUNK
    j = 0
    for c in range(n_chunks):
        for wave in range(LH_WAVES):
            for t in range(2):
                cb[base + c * LH_CHUNK + (3 * t + 1) * LH_THREADS + wave * 64 + (5 * wave + 11 * t) % 64] = cold[j % len(cold)]
                j += 1
    for j, c in enumerate(crowd):
        cb[base + LH_CHUNK + 64 * j + 3] = c          # chunk 1 behind X's chunks, waves 0..4, item 0
    # misses: keys not on the list (some have a neighbour on it) and reads with an N
    for t in range(600):
        i = base + 2 * LH_CHUNK + 13 * t
        cb[i] = int(wl[20000 + 31 * t]) ^ (1 if t % 2 else 0x300)
        if t % 5 == 0:
            cb[i] &= 0x3FFFFFFF
            qualn[i, 0] |= 0x80
            flags[i] |= FLAG_HAS_N
    env = {}
    target = None
    if cold_cap is not None:
        env["CRGPU_COLD_CAP"] = str(cold_cap)
        target = (len(x_hits) + 3, 9)                 # (chunk behind `first`, wave)
        for t in range(cold_cap + cold_surplus):
            cb[first + target[0] * LH_CHUNK + (t % LH_ITEMS) * LH_THREADS + target[1] * 64 + 20 + t // LH_ITEMS] = cold[(7 * t) % len(cold)]
        cb[first + target[0] * LH_CHUNK + 1 * LH_THREADS + target[1] * 64 + (5 * target[1]) % 64] = top      # (the two regular ones of that wave)
        cb[first + target[0] * LH_CHUNK + 4 * LH_THREADS + target[1] * 64 + (5 * target[1] + 11) % 64] = top
    name = "table_2^%d%s" % (k, "" if full else "-1") + ("" if cold_cap is None else "_cold_%d_plus_%d" % (cold_cap, cold_surplus))
    case = Case(name, L, wl, {0: (wl, None)}, cb, qualn, flags, hot=True, env=env)
    case.X, case.top, case.crowd, case.x_hits, case.cnt_max = X, top, crowd, x_hits, cnt_max
    cl = case.claims
    cl.append(dict(kind="counted_rounds", cnt_shift=shift, min_shift=19))
    cl.append(dict(kind="top_rank", key=top, rank=n_list - 1, rank_mask_minus_one=not full))
    cl.append(dict(kind="alone_in_buckets", key=X))
    cl.append(dict(kind="chunk_hits", key=X, hits=x_hits, cnt_max=cnt_max))
    cl.append(dict(kind="crowd", keys=crowd))
    if cold_cap is not None:
        cl.append(dict(kind="cold_wave", chunk=target[0], wave=target[1], count=cold_cap + cold_surplus, others_below=cold_cap))
    return case


# ---- group A: the exact lookup ------------------------------------------------------------------------------------------
def clustered_case(L, hot):
    """Bins of the exact index with 1, 7, 8, 9 and more keys, each size starting at an odd and at an even offset; the last bin
    ends the table and holds the all-T key.  Every listed barcode is read, and in every bin a key that is not listed.  16 bases:
    a bin is a head (65536 tails); 5 bases: a bin is the top 6 bits (16 keys)."""
    n = N_TABLE
    rng = np.random.default_rng(31 + L)
    low_bits, big = (16, 20) if L == 16 else (4, 12)
    n_bins = 1 << (2 * L - low_bits)
    sizes = [1, 7, 8, 9, big, 1, 7, 8, 9, big]
    bins = sorted(set(int(x) for x in np.linspace(1, n_bins - 3, len(sizes) - 1).astype(int))) + [n_bins - 1]
    assert len(bins) == len(sizes)
    wl, near = [], []
    for bn, sz in zip(bins, sizes):
        lows = sorted(int(x) for x in rng.choice((1 << low_bits) - 1, sz + 1, replace=False))      # (all ones is not drawn)
        spare = lows.pop(sz // 2)                    # not listed, between listed ones
        if bn == n_bins - 1:
            lows[-1] = (1 << low_bits) - 1           # all T
        wl += [(bn << low_bits) | t for t in lows]
        near.append((bn << low_bits) | spare)
    wl = np.array(sorted(set(wl)), U32)
    near += [((bn + 1) << low_bits) | 5 for bn in bins[:-1]]          # keys in empty bins
    near = np.array([k for k in near if k not in set(wl.tolist())], U32)
    rk = Reads(n, L, wl, rng)
    first = first_of(n)
    if hot:
        rk.cb[:first] = wl[0]      # the table holds one barcode: behind the sampling batch every other hit takes the cold queue
    both = np.concatenate([wl, near])
    for j, k in enumerate(both):
        rk.put(first + 3 + 29 * j, int(k))
        rk.put(first + LH_CHUNK + 7 + 13 * j, int(k))
        if not hot or j >= len(wl):
            rk.put(5 + 3 * j, int(k))
    # reads with an N at the last base whose completions are the last keys of the long bins: wl_lookup from pass B
    lay = ListLayout(wl, L)
    tails = [int(wl[hi - 1 - t]) for lo, hi in zip(lay.offE[:-1], lay.offE[1:]) if hi - lo > 7 for t in (0, 1)]
    for j, k in enumerate(tails):
        rk.put(n - 100 - 3 * j, k & ~3, n_at=(L - 1,))
    case = Case("clustered_L%d%s" % (L, "_table" if hot else ""), L, wl, {0: (wl, None)}, rk.cb, rk.qualn, rk.flags, thresh=0.5, hot=hot)
    case.claims.append(dict(kind="exact_bins", sizes=sorted(set(sizes)), low_bits=low_bits))
    case.claims.append(dict(kind="every_key_read", near=len(near)))
    case.claims.append(dict(kind="n_completions_behind_the_first_load", at_least=6))
    if hot:
        case.claims.append(dict(kind="cold_long_bins", sizes=[8, 9, big]))
    return case


def one_barcode_case(n_list, rank, n):
    """every read is the barcode of `rank`: with n a multiple of MB_TILE its bucket's staging region is filled to the last entry"""
    L = 16
    wl = spread_list(n_list)
    cb = np.full(n, wl[rank], U32)
    case = Case("one_barcode_%d_rank_%d_n_%d" % (n_list, rank, n), L, wl, {0: (wl, None)}, cb, np.full((n, L), Q0, np.uint8), np.zeros(n, np.uint8))
    case.claims.append(dict(kind="one_bucket", rank=rank, fills_cap=n % MB_TILE == 0))
    return case


def bucket_switch_case(n_list):
    """a list on one side of 31 x 32768 barcodes, a call with a table: reads on ranks 0, 32767, 32768 and the last one, misses between them"""
    L, n = 16, N_TABLE
    rng = np.random.default_rng(37)
    wl = spread_list(n_list)
    ranks = np.array([0, BIN_SIZE - 1, BIN_SIZE, n_list - 1, 30 * BIN_SIZE + 5, 31 * BIN_SIZE - 1], np.int64)
    cb = wl[ranks[rng.integers(0, len(ranks), n)]]
    miss = rng.random(n) < 0.02
    cb[miss] ^= U32(0x00030000)
    case = Case("bucket_switch_%d" % n_list, L, wl, {0: (wl, None)}, cb, np.full((n, L), Q0, np.uint8), np.zeros(n, np.uint8), hot=True)
    case.claims.append(dict(kind="buckets", staged=n_list <= SI_MISS_BUCKET * BIN_SIZE))
    case.claims.append(dict(kind="ranks_read", ranks=[0, BIN_SIZE - 1, BIN_SIZE, n_list - 1]))
    return case


# ---- group B: more buckets than the staged histogram takes ---------------------------------------------------------------
def many_buckets_case():
    """a canonical list of 68 x 32768 + 1 barcodes and fifteen libraries configured (partial lists): 69 x 15 buckets; library 15 has
    no list"""
    L, n = 16, 6000
    rng = np.random.default_rng(41)
    n_list = (MB_MAX_BUCKETS // (MAX_LIB - 1)) * BIN_SIZE + 1
    step = ((1 << 32) - 20000) // n_list
    canon = (np.arange(n_list, dtype=np.uint64) * np.uint64(step) + np.uint64(99)).astype(U32)
    libs = {}
    for l in range(MAX_LIB - 1):
        pos = np.unique(np.concatenate([[0, n_list - 1, BIN_SIZE - 1, BIN_SIZE], rng.integers(0, n_list, 300)]))
        libs[l] = (canon[pos], None)
    lib = rng.integers(0, MAX_LIB, n).astype(np.uint8)            # library 15 is not configured
    cb = np.zeros(n, U32)
    for l in range(MAX_LIB - 1):
        s = np.nonzero(lib == l)[0]
        cb[s] = libs[l][0][rng.integers(0, len(libs[l][0]), len(s))]
    s = np.nonzero(lib == MAX_LIB - 1)[0]
    cb[s] = canon[rng.integers(0, n_list, len(s))]
    off = rng.random(n) < 0.1
    cb[off] ^= U32(2)                                             # near misses
    other = rng.random(n) < 0.05
    cb[other] = canon[rng.integers(0, n_list, int(other.sum()))]  # canonical, mostly not on the read's partial list
    qualn = np.full((n, L), Q0, np.uint8)
    flags = lib.copy()
    has_n = np.nonzero(rng.random(n) < 0.03)[0]
    cb[has_n] &= U32(0x3FFFFFFF)
    qualn[has_n, 0] |= 0x80
    flags[has_n] |= FLAG_HAS_N
    case = Case("many_buckets", L, canon, libs, cb, qualn, flags, thresh=0.5)
    case.claims.append(dict(kind="plain_atomics", libs=MAX_LIB - 1))
    case.claims.append(dict(kind="mixed_call", unconfigured=MAX_LIB - 1))
    return case


# ---- the claims ---------------------------------------------------------------------------------------------------------
def _run_at(d, pos):
    """(first position, length, usable lanes) of the run of equal keys that covers sorted position pos"""
    k = d.sorted_keys
    a = pos
    while a > 0 and k[a - 1] == k[pos]:
        a -= 1
    b = pos
    while b + 1 < len(k) and k[b + 1] == k[pos]:
        b += 1
    return a, b - a + 1, int(d.sorted_usable[a:b + 1].sum())


def check_claims(case):
    """assert every claim of the case against its recomputed structure; returns the structure"""
    d = describe(case)
    e = expected(case)
    L = case.L
    assert case.claims, case.name
    for c in case.claims:
        kind = c["kind"]
        if kind == "behind_first":
            assert d.table and min(c["reads"]) >= d.first and (e.idx_a[c["reads"]] == MISS).all()
        elif kind == "ratio":
            r, _ = read_numbers(case, c["read"])
            assert r == c["value"] and len(candidates(case, c["read"])) == c["n_cand"], (case.name, c, r)
        elif kind == "tie_orders":      # the larger rank is the candidate met second in one read, the one met first in the other
            order = [candidates(case, i) for i in c["reads"]]
            assert sorted(o[1][1] > o[0][1] for o in order) == [False, True] and all(o[0][0] < o[1][0] for o in order)
        elif kind == "ratio_above":
            assert read_numbers(case, c["read"])[0] > c["value"]
        elif kind == "expected_order":
            s = [read_numbers(case, i)[1] for i in c["reads"]]
            assert all(a < b for a, b in zip(s, s[1:])), s
        elif kind == "priors":
            assert sorted(int(case.prior[r]) for _, r in candidates(case, c["read"])) == sorted(c["values"])
        elif kind == "n_cand":
            got = candidates(case, c["read"])
            assert len(got) == c["count"], (case.name, c, got)
            if c.get("slots") is not None:
                assert [s for s, _ in got] == c["slots"], (case.name, c, got)
        elif kind == "has_slots":
            assert set(c["slots"]) <= set(s for s, _ in candidates(case, c["read"]))
        elif kind == "same_key":
            a, b = c["reads"]
            assert case.cb[a] == case.cb[b] and (case.flags[a] ^ case.flags[b]) & FLAG_HAS_N and e.idx_b[a] != e.idx_b[b]
        elif kind == "larger_rank_is_smaller_raw":
            (s1, r1), (s2, r2) = candidates(case, c["read"])
            ks, rs = case.rank_tables(0)
            raw = {int(r): int(k) for k, r in zip(ks, rs)}
            assert (r1 > r2) == (raw[r1] < raw[r2])
        elif kind == "sorted_total":
            assert d.table and len(d.sorted_keys) == c["total"], (case.name, len(d.sorted_keys), c)
        elif kind == "all_corrected":
            assert int(e.corrected.sum()) == c["count"]
        elif kind == "chunk_runs":
            runs = sorted_chunks(d)[c["chunk"]]
            assert len(runs) == c["runs"], (case.name, c, len(runs))
            if "wanted" in c:
                assert sum(1 for r in runs if r[2] > 0) == c["wanted"]
        elif kind == "run":
            a, ln, us = _run_at(d, c["pos"])
            assert (a, ln, us, a % 64) == (c["pos"], c["length"], c["length"], c["lane"]), (case.name, c, a, ln, us)
            assert e.corrected[d.sorted_reads[a:a + ln]].all()
        elif kind == "run_in_wave":
            assert (c["pos"] // 64) % KS_WAVES == c["wave"] and c["pos"] % 64 == 0
        elif kind == "indexless_head":
            a, ln, us = _run_at(d, c["pos"])
            assert a == c["pos"] and not d.sorted_usable[a] and us == c["usable"] and d.sorted_usable[a + 1:a + ln].all()
            assert e.corrected[d.sorted_reads[a + 1:a + ln]].all()
        elif kind == "indexless_batch":
            runs = sorted_chunks(d)[c["chunk"]]
            assert len(runs) > KS_HEADS and all(r[2] == 0 for r in runs[:KS_HEADS]) and any(r[2] > 0 for r in runs[KS_HEADS:])
        elif kind == "run_disagrees":
            a, ln, us = _run_at(d, c["pos"])
            got = e.idx_b[d.sorted_reads[a:a + ln]]
            assert a == c["pos"] and ln == len(c["pattern"]) and (got != MISS).all() and len(set(got.tolist())) == 2
            assert [int(g != got[0]) for g in got] == c["pattern"]
        elif kind == "bins":
            lay = d.lists[0]
            seen = set()
            for key, us in zip(d.sorted_keys, d.sorted_usable):
                if us:
                    lo, hi = lay.binA(key) if c["table"] == "A" else lay.binB(key)
                    seen.add((hi - lo, lo & 1))
            want = set((s, p) for s in c["sizes"] if s for p in (0, 1))
            assert want <= seen and any(s == 0 for s, _ in seen), (case.name, c, sorted(want - seen))
            assert "also" not in c or any(s == c["also"] for s, _ in seen)
        elif kind == "items_in_batch":
            lay = d.lists[0]
            runs = sorted_chunks(d)[c["chunk"]][:KS_HEADS]
            items = 0
            for a, ln, us, _ in runs:
                for lo, hi in (lay.binA(d.sorted_keys[c["chunk"] * 64 + a]), lay.binB(d.sorted_keys[c["chunk"] * 64 + a])):
                    items += (hi - (lo & ~1) + 7) // 8 if hi > lo else 0
            assert items > c["more_than"]
        elif kind == "region_counts":
            for r, cnt in c["counts"].items():
                assert d.rec_count[r] == cnt, (case.name, r, d.rec_count[r], cnt)
            assert d.rec_count.sum() == sum(c["counts"].values())
        elif kind == "n_queue":
            # the queue of one wave of the part's workgroup: 256 records per step, 64 of them this wave's; drained at 64
            cnt = int(d.rec_count[c["region"]])
            lo, hi = cnt * c["part"] // K2_PARTS, cnt * (c["part"] + 1) // K2_PARTS
            is_n = (case.flags[d.rec_reads[int(d.rec_count[:c["region"]].sum()):][lo:hi]] & FLAG_HAS_N) != 0
            qn = peak = 0
            for p0 in range(0, hi - lo, 256):
                qn += int(is_n[p0 + 64 * c["wave"]:p0 + 64 * c["wave"] + 64].sum())
                peak = max(peak, qn)
                qn -= 64 if qn >= 64 else 0
            assert peak == c["peak"], (case.name, c, peak)
        elif kind == "empty_parts":
            cnt = int(d.rec_count[c["region"]])
            assert sum(1 for p in range(K2_PARTS) if cnt * p // K2_PARTS == cnt * (p + 1) // K2_PARTS) == c["empty"]
        elif kind == "buckets":
            assert (d.buckets_per_lib <= SI_MISS_BUCKET) == c["staged"] and abs(d.buckets_per_lib - SI_MISS_BUCKET - 0.5) < 1
        elif kind == "sampled_misses_share_keys":
            assert len(np.intersect1d(case.cb[:d.first][d.miss[:d.first]], case.cb[d.rec_reads])) >= c["at_least"]
        elif kind == "fullest_region":
            assert d.rec_count[c["region"]] == c["count"] and np.delete(d.rec_count, c["region"]).max() < c["others_below"]
        elif kind == "counted_rounds":
            assert d.table and d.counted and d.cnt_shift == c["cnt_shift"] >= c["min_shift"] and d.cnt_shift <= HC_MAX_RANK_BITS
        elif kind == "top_rank":
            r = int(np.searchsorted(case.canon, c["key"]))
            cnt = np.bincount(e.idx_a[e.idx_a != MISS].astype(np.int64), minlength=d.n_canon)
            assert r == c["rank"] == d.n_canon - 1 == int(cnt.argmax())
            assert (r == (1 << d.cnt_shift) - 2) == c["rank_mask_minus_one"]
        elif kind == "alone_in_buckets":
            hx = int(hot_hash([c["key"]])[0])
            hs = hot_hash(d.sampled).astype(np.int64)
            assert c["key"] in d.sampled and len(d.sampled) <= HOT_CAP
            assert sum(1 for k, h in zip(d.sampled, hs) if k != c["key"] and min((h - hx) % HOT_BUCKETS, (hx - h) % HOT_BUCKETS) <= 1) == 0
        elif kind == "chunk_hits":
            x = case.cb[d.first:] == c["key"]
            got = np.bincount(d.chunk[x], minlength=len(c["hits"]))
            assert got[:len(c["hits"])].tolist() == c["hits"] and got[len(c["hits"]):].sum() == 0
            cm = c["cnt_max"]
            assert cm == 0xFFFFFFFF >> d.cnt_shift and {cm, cm + 1, cm + 2, 2 * (cm + 1)} <= set(c["hits"])
        elif kind == "crowd":
            hs = set(hot_hash(c["keys"]).tolist())
            assert len(hs) == 1 and len(c["keys"]) == 5 and set(c["keys"]) <= set(d.sampled.tolist())
            h0 = hs.pop()
            assert sum(1 for h in hot_hash(d.sampled) if h in (h0, (h0 - 1) % HOT_BUCKETS)) == 5       # nobody else wants those four slots
            assert all((case.cb[d.first:] == k).any() for k in c["keys"])
        elif kind == "cold_wave":
            cold = ~d.miss[d.first:] & ~np.isin(case.cb[d.first:], d.sampled)
            maybe = np.isin(case.cb[d.first:], case.crowd)
            per = np.bincount(d.region[cold | maybe], minlength=REGIONS)
            tgt = c["chunk"] * LH_WAVES + c["wave"]
            assert np.bincount(d.region[cold], minlength=REGIONS)[tgt] == per[tgt] == c["count"]
            assert np.delete(per, tgt).max() < c["others_below"]
        elif kind == "exact_bins":
            lay = d.lists[0]
            sz = np.diff(lay.offE)
            seen = set((int(s), int(lo) & 1) for s, lo in zip(sz, lay.offE[:-1]) if s)
            assert lay.shiftE == c["low_bits"]
            assert set((s, p) for s in c["sizes"] for p in (0, 1) if s > 1) <= seen, (case.name, sorted(seen))
            assert sz[-1] > 0 and int(lay.keys[-1]) == (1 << (2 * L)) - 1      # the last bin ends the table, with the all-T key
        elif kind == "every_key_read":
            assert np.isin(case.libs[0][0], case.cb).all() and int(d.miss.sum()) >= c["near"]
            lay = d.lists[0]
            bins_missed = set(int(k) >> lay.shiftE for k in case.cb[d.miss])
            assert set(np.nonzero(np.diff(lay.offE))[0].tolist()) <= bins_missed
        elif kind == "n_completions_behind_the_first_load":      # listed completions of N reads at bin positions the 16-byte load misses
            lay = d.lists[0]
            n = 0
            for i in np.nonzero(case.flags & FLAG_HAS_N)[0]:
                for _, r in candidates(case, i):
                    lo, hi = lay.binE(int(case.canon[r]))
                    n += int(r >= (lo & ~1) + 8)
            assert n >= c["at_least"], (case.name, n)
        elif kind == "cold_long_bins":      # hits the table cannot answer, in bins of more than 7 keys at both parities
            lay = d.lists[0]
            cold = np.unique(case.cb[d.first:][~d.miss[d.first:] & ~np.isin(case.cb[d.first:], d.sampled)])
            seen = set((hi - lo, lo & 1) for lo, hi in (lay.binE(k) for k in cold))
            assert len(d.sampled) == 1 and set((s, p) for s in c["sizes"] for p in (0, 1)) <= seen, (case.name, sorted(seen))
        elif kind == "one_bucket":
            assert (e.idx_a == c["rank"]).all() and (case.n % MB_TILE == 0) == c["fills_cap"]
        elif kind == "ranks_read":
            assert set(c["ranks"]) <= set(e.idx_a.tolist())
        elif kind == "plain_atomics":
            assert len(case.libs) == c["libs"] and d.buckets_per_lib * len(case.libs) > MB_MAX_BUCKETS
        elif kind == "mixed_call":
            lib = case.flags & FLAG_LIB_MASK
            assert len(np.unique(lib)) == MAX_LIB and c["unconfigured"] not in case.libs and (lib == c["unconfigured"]).any()
            assert ((case.flags & FLAG_HAS_N) != 0).any()
        else:
            raise AssertionError("unknown claim %r" % kind)
    return d


# ---- the catalogue ------------------------------------------------------------------------------------------------------
LIST_31 = SI_MISS_BUCKET * BIN_SIZE          # the largest list whose ranks the staged histogram of k_stage_idx takes
TABLE_K = 20                                 # 2^20 - 1 and 2^20 barcodes: hit fields of 12 and 11 bits

BUILDERS = {
    "decision": lambda: decision_case(False),
    "decision_translated": lambda: decision_case(True),
    "sorted": sorted_case,
    "sorted_total_1": lambda: sorted_total_case(1),
    "sorted_total_64": lambda: sorted_total_case(64),
    "sorted_total_65": lambda: sorted_total_case(65),
    "dense8": dense8_case,
    "records_31": lambda: records_case(LIST_31, "records_31"),
    "records_32": lambda: records_case(LIST_31 + 1, "records_32"),
    "records_big": records_big_case,
    "record_cap_exact": lambda: record_cap_case(7, 0),
    "record_cap_plus_one": lambda: record_cap_case(7, 1),
    "table_odd": lambda: table_case(TABLE_K, False),
    "table_full": lambda: table_case(TABLE_K, True),
    "table_cold_exact": lambda: table_case(TABLE_K, True, cold_cap=5, cold_surplus=0),
    "table_cold_plus_one": lambda: table_case(TABLE_K, True, cold_cap=5, cold_surplus=1),
    "clustered_L16": lambda: clustered_case(16, False),
    "clustered_L16_table": lambda: clustered_case(16, True),
    "clustered_L5": lambda: clustered_case(5, False),
    "one_barcode_full": lambda: one_barcode_case(LIST_31, BIN_SIZE - 1, 2 * MB_TILE),
    "one_barcode_plus_one": lambda: one_barcode_case(LIST_31 + 1, BIN_SIZE, 2 * MB_TILE + 1),
    "bucket_switch_31": lambda: bucket_switch_case(LIST_31),
    "bucket_switch_32": lambda: bucket_switch_case(LIST_31 + 1),
    "many_buckets": many_buckets_case,
}
_cache = {}


def get_case(name):
    if name not in _cache:
        _cache[name] = BUILDERS[name]()
    return _cache[name]
