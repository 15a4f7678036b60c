"""Direct differential test of the key build (csrc/keys.hip: k_build_keys, k_build_keys_v4, build_keys_impl) through
Context.build_keys.  The expectation is a numpy model of what a read's key is:

    keep = UMI valid, and idx != MISS, and feature != NO_FEATURE, and feature < n_features, and lib < n_libs
           (and, with per-read UMI lengths, umi_min_len <= length <= umi_len)
    key  = b << sh_bc | f << sh_feat | lib << sh_libid | (L - Lc) << sh_lib | umi << 1 | nontx

with the field widths of crgpu_set_key_layout.  UMI validity is the oracle's umi_is_valid (pinned to the reference's vectors),
asked once per (UMI, quality row) pattern of a small pool that the reads draw from.  The unordered kernels emit in arrival
order, so the device's keys are sorted on the host and compared as a multiset, together with n_keys; order is covered by the
DupInfo of count_records.  Histograms are checked the way the sort consumes them: counts with and without them agree."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_WL, N_FEATURES, N_LIBS = 1000, 37, 3
SIZES_SCALAR = (1, 3, 4, 255, 256, 257, 4095)                  # one chunk of the scalar kernel, partial chunk
SIZES_V4 = (4096, 4097, 4098, 4099, 8191, 8192, 12289)        # four reads per lane, tails of 0 - 3 reads, the chunk edge
# (umi_len, umi_min_len): dword quality rows (LQW 1 - 4), the byte path, per-read lengths 9 .. 13 of which 9 and 13 drop the read
UMI_CONFIGS = ((4, None), (8, None), (12, None), (16, None), (5, None), (10, None), (12, 10))
SENTINEL = np.uint64(0xDEADBEEFDEADBEEF)

# what is planted: name -> does the read survive it
KINDS = (("miss", False), ("no_feature", False), ("feature_eq_n", False), ("lib_eq_n", False), ("n_first", False),
         ("n_last", False), ("q_star", False), ("q_plus", True), ("q_32", True), ("homopolymer", False), ("neighbour", True),
         ("nontx", True))
UMI_KINDS = ("n_first", "n_last", "q_star", "q_plus", "q_32", "homopolymer", "neighbour")
N_RANDOM = 40  # random patterns of the pool per length, in front of the planted ones

_ctxs = {}


def _ctx(dense):
    import gpu_helpers as G
    from cellranger_amd import synth as S

    if dense not in _ctxs:
        c = G.fresh_ctx(trust=False, dense=dense)
        c.set_whitelist(0, S.Workload(n_total=1000, seed=1, n_wl=N_WL, n_cells=10, n_ambient=10).wl_packed, length=16)
        _ctxs[dense] = c
    return _ctxs[dense]


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for c in _ctxs.values():
        c.close()
    _ctxs.clear()


@functools.lru_cache(maxsize=None)
def _pool(L, lo):
    """The (UMI, quality row) patterns the reads draw from, for every UMI length lo .. L: packed UMI, length, quality
    row of L bytes (bit 7 = N, zero behind the length), and the oracle's verdict on each.  pool["special"][(kind, length)]
    is the index of a planted pattern."""
    import oracle_lib as O

    rng = np.random.default_rng(1000 * L + lo)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    bases, quals, special = [], [], {}
    for Lp in range(lo, L + 1):
        for _ in range(N_RANDOM):
            bases.append(rng.integers(0, 4, Lp))
            quals.append(rng.integers(43, 74, Lp).astype(np.uint8))       # '+' .. 'I': never below UMI_MIN_QV
        for kind in UMI_KINDS:
            b, q = rng.integers(0, 4, Lp), np.full(Lp, 70, np.uint8)
            b[0], b[-1] = 1, 2                                            # not a homopolymer (for Lp >= 2)
            if kind == "n_first":
                q[0] |= 0x80
            elif kind == "n_last":
                q[-1] |= 0x80
            elif kind == "q_star":
                q[rng.integers(0, Lp)] = 42                               # '*': 42 - 33 = 9
            elif kind == "q_plus":
                q[:] = 43                                                 # '+': 10
            elif kind == "q_32":
                q[rng.integers(0, Lp)] = 32                               # 32 - 33 wraps to 255
            elif kind == "homopolymer":
                b[:] = 2
            elif kind == "neighbour":                                     # the homopolymer but for its last base
                b[:] = 2
                b[-1] = 3
            special[(kind, Lp)] = len(bases)
            bases.append(b)
            quals.append(q)
    n = len(bases)
    length = np.array([len(b) for b in bases], np.uint32)
    packed = np.array([sum(int(x) << (2 * (len(b) - 1 - k)) for k, x in enumerate(b)) for b in bases], np.uint32)
    qrow = np.zeros((n, L), np.uint8)
    valid = np.zeros(n, bool)
    for i, (b, q) in enumerate(zip(bases, quals)):
        qrow[i, :len(q)] = q
        seq = np.where(q & 0x80, ord("N"), acgt[b]).astype(np.uint8)
        valid[i] = O.umi_is_valid(seq.tobytes(), q & 0x7F)
    for (kind, Lp), i in special.items():                                 # the verdicts the planted patterns are there for
        assert valid[i] == dict(KINDS)[kind], (kind, Lp)
    assert valid[:N_RANDOM].sum() >= N_RANDOM - 2                         # random UMIs are valid but for a chance homopolymer
    return dict(packed=packed, length=length, qrow=qrow, valid=valid, special=special, n=n)


def _positions(n):
    n4 = n & ~3
    return sorted({p for p in (0, 255, 256, 4095, 4096, n4 - 1, n4, n - 1) if 0 <= p < n})


def _reads(n, L, lo, seed, mode="random"):
    """Read arrays of one input.  mode: "random" (every kind of read at random), "kept" (every read survives), "none" (every
    read is rejected, each for one reason)."""
    pool = _pool(L, lo or L)
    rng = np.random.default_rng(seed)
    var = lo is not None
    rd = dict(n=n, L=L, lo=lo)
    rd["idx"] = rng.integers(0, N_WL, n).astype(np.uint32)
    rd["feature"] = rng.integers(0, N_FEATURES, n).astype(np.uint32)
    rd["flags"] = rng.integers(0, N_LIBS, n).astype(np.uint8)
    rd["ulen"] = (rng.integers(lo, L + 1, n) if var else np.full(n, L)).astype(np.uint8)
    valid_of = {Lp: np.flatnonzero(pool["valid"] & (pool["length"] == Lp)) for Lp in range(lo or L, L + 1)}
    all_of = {Lp: np.flatnonzero(pool["length"] == Lp) for Lp in range(lo or L, L + 1)}
    pick = all_of if mode == "random" else valid_of            # chosen before any length leaves the range below
    rd["pattern"] = _choose(rng, pick, rd["ulen"])
    if mode == "random":
        from cellranger_amd._lib import FLAG_NONTXOMIC, MISS, NO_FEATURE

        u = rng.random(n)
        rd["idx"][u < 0.05] = MISS
        u = rng.random(n)
        rd["feature"][u < 0.05] = NO_FEATURE
        rd["feature"][(u >= 0.05) & (u < 0.07)] = N_FEATURES
        rd["feature"][(u >= 0.07) & (u < 0.08)] = N_FEATURES + 5
        rd["flags"][rng.random(n) < 0.02] = N_LIBS
        rd["flags"] |= np.where(rng.random(n) < 0.3, FLAG_NONTXOMIC, 0).astype(np.uint8)
        if var:   # lengths outside umi_min_len .. umi_len: no UMI
            u = rng.random(n)
            rd["ulen"][u < 0.03] = lo - 1
            rd["ulen"][(u >= 0.03) & (u < 0.06)] = L + 1
    elif mode == "none":
        for i in range(n):
            _plant(rd, i, [k for k, survives in KINDS if not survives][i % 8])
    return rd


def _choose(rng, pick, ulen):
    out = np.zeros(len(ulen), np.int64)
    for Lp, cand in pick.items():
        m = ulen == Lp
        out[m] = rng.choice(cand, int(m.sum()))
    return out


def _plant(rd, i, kind):
    from cellranger_amd._lib import FLAG_NONTXOMIC, MISS, NO_FEATURE

    L, lo = rd["L"], rd["lo"]
    if kind == "miss":
        rd["idx"][i] = MISS
    elif kind == "no_feature":
        rd["feature"][i] = NO_FEATURE
    elif kind == "feature_eq_n":
        rd["feature"][i] = N_FEATURES
    elif kind == "lib_eq_n":
        rd["flags"][i] = (rd["flags"][i] & 0xF0) | N_LIBS
    elif kind == "nontx":
        rd["flags"][i] |= FLAG_NONTXOMIC
    else:
        if not (lo or L) <= rd["ulen"][i] <= L:
            rd["ulen"][i] = L
        rd["pattern"][i] = _pool(L, lo or L)["special"][(kind, int(rd["ulen"][i]))]


def _plant_all(rd, rot):
    """every kind at once: the kinds rotate over the planted positions"""
    for q, p in enumerate(_positions(rd["n"])):
        _plant(rd, p, KINDS[(q + rot) % len(KINDS)][0])


def _layout(L, lo, bits_bc):
    cl2 = lambda x: int(np.ceil(np.log2(x))) if x > 1 else 0
    bits_ulen = cl2(L - lo + 1) if lo is not None else 0
    sh_lib = 1 + 2 * L
    sh_libid = sh_lib + bits_ulen
    sh_feat = sh_libid + cl2(N_LIBS)
    return dict(sh_lib=sh_lib, sh_libid=sh_libid, sh_feat=sh_feat, sh_bc=sh_feat + cl2(N_FEATURES), bits=sh_feat + cl2(N_FEATURES) + bits_bc)


def _device_arrays(rd, rng):
    """what is uploaded: the packed UMI carries random bits above its 2 * length bits (the kernel masks them)"""
    pool = _pool(rd["L"], rd["lo"] or rd["L"])
    plen = pool["length"][rd["pattern"]]
    junk = rng.integers(0, 1 << 32, rd["n"], dtype=np.uint64) << (2 * plen).astype(np.uint64)
    umi = ((pool["packed"][rd["pattern"]].astype(np.uint64) | junk) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    return dict(idx=rd["idx"], umi=umi, uq=pool["qrow"][rd["pattern"]], feature=rd["feature"], flags=rd["flags"], ulen=rd["ulen"])


def _model_keys(rd, with_flags=True, columns=None):
    """sorted keys of the kept reads.  columns: rank -> column of the BarcodeIndex under CRGPU_OPT_DENSE_BARCODE_KEYS"""
    from cellranger_amd._lib import FLAG_NONTXOMIC, MISS, NO_FEATURE

    L, lo = rd["L"], rd["lo"]
    pool = _pool(L, lo or L)
    fl = rd["flags"] if with_flags else np.zeros(rd["n"], np.uint8)
    lib = (fl & 0x0F).astype(np.uint64)
    Li = rd["ulen"].astype(np.int64)
    in_range = (Li >= (lo or L)) & (Li <= L)
    keep = pool["valid"][rd["pattern"]] & (rd["idx"] != MISS) & (rd["feature"] != NO_FEATURE) & (rd["feature"] < N_FEATURES) & \
        (lib < N_LIBS) & in_range
    if columns is None:
        b, bits_bc = rd["idx"].astype(np.uint64), int(np.ceil(np.log2(N_WL)))
    else:
        b = np.searchsorted(columns, rd["idx"]).astype(np.uint64)
        bits_bc = max(1, int(np.ceil(np.log2(len(columns)))))
    lay = _layout(L, lo, bits_bc)
    assert lay["bits"] <= 64
    u = lambda x: np.uint64(x)
    key = (b << u(lay["sh_bc"])) | (rd["feature"].astype(np.uint64) << u(lay["sh_feat"])) | (lib << u(lay["sh_libid"])) | \
        ((L - np.where(in_range, Li, L)).astype(np.uint64) << u(lay["sh_lib"])) | \
        (pool["packed"][rd["pattern"]].astype(np.uint64) << u(1)) | ((fl & FLAG_NONTXOMIC) != 0).astype(np.uint64)
    return np.sort(key[keep])


def _set_layout(c, L, lo):
    c.set_key_layout(N_FEATURES, L, N_LIBS, 0)
    if lo is not None:
        c.set_umi_min_len(lo)


class _Uploaded:
    """the record arrays of one input on the device; shift = 4: every record pointer is passed 4 bytes into its buffer"""

    def __init__(self, c, rd, shift=0, seed=0):
        a = _device_arrays(rd, np.random.default_rng(seed))
        self.c, self.rd, self.n, self.shift = c, rd, rd["n"], shift
        self.buf = {}
        for k, v in a.items():
            raw = np.ascontiguousarray(v).view(np.uint8).reshape(-1)
            self.buf[k] = c.upload(np.concatenate([np.zeros(shift, np.uint8), raw]))

    def records(self, with_flags=True):
        p = {k: b.ptr + self.shift for k, b in self.buf.items()}
        return self.c.records(self.n, self.rd["L"], p["idx"], p["umi"], p["uq"], p["feature"], p["flags"] if with_flags else None,
                              d_umi_len=p["ulen"] if self.rd["lo"] is not None else None)


def _check_build(c, up, with_flags, trust, columns=None):
    """one crgpu_build_keys_dev call against the model: n_keys, the multiset of keys, nothing written behind them"""
    n = up.n
    c.trust_unchanged_buffers(trust)
    d_keys = c.upload(np.full(n + 8, SENTINEL, np.uint64))
    nk = c.build_keys(up.records(with_flags), d_keys)
    exp = _model_keys(up.rd, with_flags, columns)
    got = d_keys.to_host()
    what = (n, up.rd["L"], up.rd["lo"], with_flags, trust)
    assert nk == len(exp), what
    assert np.array_equal(np.sort(got[:nk]), exp), what
    assert (got[nk:] == SENTINEL).all(), what
    return nk


@pytest.mark.parametrize("L,lo", UMI_CONFIGS)
def test_every_size_and_umi_length_against_the_model(L, lo):
    """Random reads of every kind with every planted kind at once at the reads 0, 255, 256, 4095, 4096, n4 - 1, n4, n - 1; each
    with and without the histograms (trust_unchanged_buffers) and with d_flags given and None."""
    c = _ctx(False)
    _set_layout(c, L, lo)
    for k, n in enumerate(SIZES_SCALAR + SIZES_V4):
        rd = _reads(n, L, lo, seed=7 * n + L)
        _plant_all(rd, rot=k)
        up = _Uploaded(c, rd, seed=n)
        kept = [_check_build(c, up, wf, trust) for wf in (True, False) for trust in (False, True)]
        assert n < 255 or 0 < min(kept) <= max(kept) < n


@pytest.mark.parametrize("kind,survives", KINDS)
def test_one_planted_kind_at_the_chunk_and_vector_edges(kind, survives):
    """Every read is kept but the planted ones: n_keys tells whether exactly those were dropped.  Scalar kernel (257 reads), four
    reads per lane with a tail of three (4099), dword rows (UMI 12) and the byte path (UMI 5, UMI 12 with per-read lengths)."""
    c = _ctx(False)
    for L, lo in ((12, None), (5, None), (12, 10)):
        _set_layout(c, L, lo)
        for n in (257, 4099):
            rd = _reads(n, L, lo, seed=n + L, mode="kept")
            pos = _positions(n)
            for p in pos:
                _plant(rd, p, kind)
            up = _Uploaded(c, rd)
            for with_flags in (True, False):
                for trust in (False, True):
                    nk = _check_build(c, up, with_flags, trust)
                    dropped = not survives and (with_flags or kind != "lib_eq_n")   # without d_flags every read is of library 0
                    assert nk == n - (len(pos) if dropped else 0)


@pytest.mark.parametrize("L,lo", [(12, None), (10, None), (12, 10)])
def test_nothing_kept_and_everything_kept(L, lo):
    c = _ctx(False)
    _set_layout(c, L, lo)
    for n in (3, 257, 4099, 8192):
        for mode in ("none", "kept"):
            up = _Uploaded(c, _reads(n, L, lo, seed=n, mode=mode))
            for trust in (False, True):
                assert _check_build(c, up, True, trust) == (n if mode == "kept" else 0)


def test_misaligned_records_take_the_scalar_kernel():
    """Every record pointer 4 bytes into its buffer: no 16-byte loads, the same keys (4099 reads, where k_build_keys_v4 would run)."""
    c = _ctx(False)
    _set_layout(c, 12, None)
    rd = _reads(4099, 12, None, seed=5)
    _plant_all(rd, rot=3)
    up = _Uploaded(c, rd, shift=4)
    assert all(b.ptr % 16 == 0 for b in up.buf.values())
    for with_flags in (True, False):
        for trust in (False, True):
            _check_build(c, up, with_flags, trust)


def test_dense_barcode_keys():
    """CRGPU_OPT_DENSE_BARCODE_KEYS: the barcode field holds the column of the rank among the ranks with a count in the tables."""
    from cellranger_amd._lib import COUNTS_VALID, MISS

    c = _ctx(True)
    for L, lo in ((12, None), (5, None)):
        for n in (257, 4099, 12289):
            rd = _reads(n, L, lo, seed=3 * n + L)
            _plant_all(rd, rot=n % 5)
            rd["idx"][rd["idx"] != MISS] //= 2     # half of the ranks: columns differ from ranks
            counts = np.zeros(N_WL, np.uint32)
            counts[rd["idx"][rd["idx"] != MISS]] = 1
            counts[N_WL - 3:] = 2                  # columns without a read
            c.set_counts(0, COUNTS_VALID, counts)
            _set_layout(c, L, lo)
            up = _Uploaded(c, rd)
            for trust in (False, True):
                _check_build(c, up, True, trust, columns=np.flatnonzero(counts).astype(np.uint32))


def _counted(c, d_keys, nk):
    cnt = c.count_keys(d_keys, nk)
    out = cnt.triplets() + tuple(cnt.molecules()[k] for k in ("bc", "lib", "feature", "umi", "read_count", "utype"))
    cnt.free()
    return out


def test_histograms_as_the_sort_consumes_them():
    """Under trust_unchanged_buffers the key build hands the digit histograms of its keys to the sort.  The counts of one call,
    of two calls that write back to back into one buffer (the second adds to the first's histograms) and of two calls into
    separate buffers (the histograms start again) equal those of the same keys counted without the promise."""
    c = _ctx(False)
    _set_layout(c, 12, None)
    n = 4097
    ups = []
    for s in (1, 2):
        rd = _reads(n, 12, None, seed=90 + s)
        rd["idx"] %= 7                              # few barcodes and features: runs of equal keys, UMIs to correct
        rd["feature"] %= 3
        rd["pattern"] %= N_RANDOM
        ups.append(_Uploaded(c, rd))

    def build(trust, up, dst):
        c.trust_unchanged_buffers(trust)
        return c.build_keys(up.records(), dst)

    def run(trust):
        out = []
        one = c.empty(n + 8, np.uint64)                     # one call
        out.append(_counted(c, one, build(trust, ups[0], one)))
        both = c.empty(2 * n + 8, np.uint64)                # two calls, back to back in one buffer, counted once
        nk1 = build(trust, ups[0], both)
        nk2 = build(trust, ups[1], both.ptr + 8 * nk1)
        out.append(_counted(c, both, nk1 + nk2))
        a, b = c.empty(n + 8, np.uint64), c.empty(n + 8, np.uint64)   # two calls, separate buffers: the second call's keys, then the first's
        nka, nkb = build(trust, ups[0], a), build(trust, ups[1], b)
        out.append(_counted(c, b, nkb))
        out.append(_counted(c, a, nka))
        return out

    ref, got = run(False), run(True)
    assert len(ref[1][3]) > len(ref[0][3]) > 0 and ref[0][7].max() > 1      # molecules of both inputs; reads share molecules
    for r, g in zip(ref, got):
        for x, y in zip(r, g):
            assert np.array_equal(x, y)


@pytest.mark.parametrize("trust", [False, True])
def test_read_order_of_count_records_across_the_chunk_edge(trust):
    """The ORDERED kernels (count_records: keys with their read ordinals, in read order): 4097 reads, rejects on both sides of
    the 4096-read chunk edge and copies of one molecule's reads across it with both UmiTypes.  Per-read DupInfo equals the
    oracle's; the representative read of a molecule is its first read, so a key out of order shows."""
    import gpu_helpers as G
    import oracle_lib as O
    from cellranger_amd import engine as E
    from cellranger_amd import synth as S
    from cellranger_amd._lib import FLAG_NONTXOMIC, NO_FEATURE

    n = 4097
    w = S.Workload(n_total=n, seed=S.SEED0 + 41, n_wl=500, n_cells=6, n_ambient=20, n_genes=5, reads_per_umi=4, cb_err=0.0)
    r = w.host_reads(0, n)
    uq = r["umi_qualn"]
    umi_ascii, umi_q = S.to_ascii(r["umi"], uq, w.umi_len)
    src = max(i for i in range(3000, 4000)                  # a read with a barcode, a feature and a valid UMI
              if not (r["flags"][i] & 0x10) and r["feature"][i] != NO_FEATURE and O.umi_is_valid(umi_ascii[i].tobytes(), umi_q[i]))
    for dst, nontx in ((4094, True), (4095, False), (4096, True), (3, True)):   # one molecule on both sides of the edge
        for f in ("cb", "cb_qualn", "umi", "feature"):
            r[f][dst] = r[f][src]
        uq[dst] = uq[src]
        r["flags"][dst] = (r["flags"][src] & 0x0F) | (FLAG_NONTXOMIC if nontx else 0)
    r["feature"][[0, 255, 256, 4090, 4093]] = NO_FEATURE                        # rejects: no feature, an N, a low quality
    uq[[1, 4089], 0] |= 0x80
    uq[[2, 4092], -1] = 42
    c = G.fresh_ctx(trust=trust)
    c.set_whitelist(0, w.wl_packed, length=16)
    _, _, _, dev = G.gpu_barcode_stage(c, r, n)
    c.set_key_layout(w.n_genes, w.umi_len, 1, 0)
    recs = c.records(n, w.umi_len, dev["idx"], c.upload(r["umi"]), c.upload(r["umi_qualn"]), c.upload(r["feature"]), dev["flags"])
    d_pu, d_rc, d_fl = c.empty(n, np.uint32), c.empty(n, np.uint32), c.empty(n, np.uint8)
    c.count_records(recs, d_pu, d_rc, d_fl).free()
    fl, pu, rc = d_fl.to_host(), d_pu.to_host(), d_rc.to_host()
    res = O.run_pipeline(G.oracle_reads_from_packed(r, w.cb_len, w.umi_len), [O.Whitelist(E.unpack_seqs(w.wl_packed, w.cb_len))],
                         n_threads=2, want_dupinfo=True)
    od = res.dupinfo
    has = od["has_dupinfo"] != 0
    assert np.array_equal((fl & 1) != 0, has)
    assert np.array_equal((fl & 2) != 0, od["is_corrected"] != 0)
    assert np.array_equal((fl & 4) != 0, od["is_low_support"] != 0)
    assert np.array_equal((fl & 8) != 0, od["is_umi_count"] != 0)
    assert np.array_equal(pu[has], od["processed_umi"][has])
    assert np.array_equal(rc[has], od["read_count"][has])
    assert not rc[~has].any() and not pu[~has].any()
    assert has[[4094, 4095, 4096]].all() and not has[[0, 1, 2, 4089, 4090, 4092, 4093]].any()
    c.close()
