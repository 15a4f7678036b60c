"""GPU parity tests of the count stage, bit-for-bit against the oracle:

* the run heads per tile of the run-length pass, counted by the finishing step of the sort (k_find_descents on the keys as
  they are before the repair, every repair path adds what it changes) instead of by a pass of its own over all sorted keys;
* the per-key state of the UMI correction (st, corr, inc_all, minidx) over two calls in one context, where the second call
  gets the first call's pool blocks: corr, inc_all and minidx mean something only where the state word says so, and a
  reader that does not ask it first sees the previous call's values.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CP_ROUND = 2048  # keys a workgroup of the run-length pass takes per round (stage_common.h)
STAT_SORT_REFINISHED = 1
STAT_RL_COUNTS_FROM_FINISH = 15


def _rl_tile(n_keys):
    """keys per tile of the run-length pass: the arithmetic of cp_blocks (stage_common.h)"""
    nb = max(1, min(4096, -(-n_keys // (CP_ROUND * 4))))
    tile = -(-n_keys // nb)
    return -(-tile // CP_ROUND) * CP_ROUND


def _oracle(w, r, whitelists=None, **kw):
    import gpu_helpers as G
    import oracle_lib as O
    from cellranger_amd import engine as E

    if whitelists is None:
        whitelists = [O.Whitelist(E.unpack_seqs(w.wl_packed, w.cb_len))] * kw.get("n_lib", 1)
    return O.run_pipeline(G.oracle_reads_from_packed(r, w.cb_len, w.umi_len), whitelists, n_threads=4, want_dupinfo=True, **kw)


def _sorted_key_columns(res, r, canon_sorted):
    """The reads that reach the count stage in the order of their keys [barcode rank][feature][library][UMI][UmiType]:
    (read index, columns of the sorted keys)."""
    import gpu_helpers as G

    valid = np.flatnonzero(res.dupinfo["has_dupinfo"] != 0)
    rank = G.ranks_of(canon_sorted, res.corrected_cb[valid]).astype(np.int64)
    feat = r["feature"][valid].astype(np.int64)
    lib = (r["flags"][valid] & 0x0F).astype(np.int64)
    umi = r["umi"][valid].astype(np.int64)
    ut = ((r["flags"][valid] & 0x20) >> 5).astype(np.int64)
    order = np.lexsort((ut, umi, lib, feat, rank))
    return valid[order], (rank[order], feat[order], lib[order], umi[order], ut[order])


def _runs_above_low_bits(cols, umi_low_bits):
    """[start, end) of the runs of sorted keys that agree in everything above the low `umi_low_bits` UMI bits"""
    rank, feat, lib, umi, _ = cols
    top = umi >> umi_low_bits
    head = np.ones(len(umi), bool)
    head[1:] = (rank[1:] != rank[:-1]) | (feat[1:] != feat[:-1]) | (lib[1:] != lib[:-1]) | (top[1:] != top[:-1])
    starts = np.flatnonzero(head)
    return starts, np.append(starts[1:], len(umi))


UMI_LOW = 5  # the planted runs differ in their last 2.5 UMI bases and in the UmiType bit: they agree above the low 6 key bits
PLANTED = (8, 40, 3000, 6000)  # one run per repair path: registers, a wave, a workgroup in LDS, one lane through memory


def _heads_inputs(w, big_run, canon_sorted, whitelists=None):
    """260 K reads in the style of test_clustered_umis_and_long_runs_of_near_identical_keys, plus one run of each length of
    PLANTED laid across a multiple of the run-length tile.  The reads of a planted run take the place of the reads whose keys
    sort last, so the number of keys (hence the tile) and the positions in front of the run stay what the oracle's sorted
    keys say."""
    from cellranger_amd._lib import FLAG_NONTXOMIC

    n = w.n_total
    r = w.host_reads(0, n)
    rng = np.random.default_rng(37)
    prefix = rng.integers(0, 1 << 16, 3, dtype=np.uint32)        # three 8-base prefixes
    r["umi"] = ((prefix[rng.integers(0, 3, n)] << np.uint32(8)) | rng.integers(0, 256, n, dtype=np.uint32)).astype(np.uint32)
    assert not (r["flags"][0] & 0x10) and not (r["cb_qualn"][0] & 0x80).any() and not (r["umi_qualn"][0] & 0x80).any()
    r["cb"][:big_run], r["feature"][:big_run] = r["cb"][0], 7
    r["cb_qualn"][:big_run], r["umi_qualn"][:big_run] = r["cb_qualn"][0], r["umi_qualn"][0]
    r["umi"][:big_run] = (r["umi"][0] & ~np.uint32(31)) | rng.integers(0, 32, big_run, dtype=np.uint32)
    r["flags"][:big_run] = r["flags"][0] & 0x0F
    r["flags"] = (r["flags"] | np.where(rng.random(n) < 0.4, FLAG_NONTXOMIC, 0)).astype(np.uint8)

    res = _oracle(w, r, whitelists)
    reads, cols = _sorted_key_columns(res, r, canon_sorted)
    n_keys = len(reads)
    tile = _rl_tile(n_keys)
    exact = res.bc_state[reads] == 1                       # anchors and donors: barcodes that are on the whitelist as read
    in_big = reads < big_run
    big_pos = np.flatnonzero(in_big)
    donors_needed = sum(PLANTED)
    donor_pos = np.flatnonzero(exact & ~in_big)[-donors_needed:]
    limit = donor_pos[0]                                    # the planted runs lie in front of every donor
    # tile multiples far from the big run, in front of the donors, a few tiles apart
    free = [t for t in range(tile, limit - max(PLANTED) - sum(PLANTED), tile)
            if t + tile < big_pos[0] or t - tile - sum(PLANTED) > big_pos[-1]]
    assert len(free) >= 2 * len(PLANTED), "not enough tile boundaries clear of the big run"
    targets = free[1::2][:len(PLANTED)]
    shift, used = 0, 0
    for length, t in zip(PLANTED, targets):
        # the planted run takes positions [p, p + length) of the new order: p = t - length / 2; it replaces the key that sits
        # at p - shift in the old order (the earlier runs moved it back by `shift`) and comes to lie around it
        p_old = t - length // 2 - shift
        while not exact[p_old] or in_big[p_old]:
            p_old -= 1
        a = reads[p_old]
        assert not (r["flags"][a] & 0x10) and not (r["umi_qualn"][a] & 0x80).any()
        d = np.append(reads[donor_pos[used:used + length - 1]], a)   # the anchor itself belongs to the run
        used += length - 1
        for f in ("cb", "feature"):
            r[f][d] = r[f][a]
        r["cb_qualn"][d], r["umi_qualn"][d] = r["cb_qualn"][a], r["umi_qualn"][a]
        r["flags"][d] = (r["flags"][a] & 0x0F) | (r["flags"][d] & FLAG_NONTXOMIC)
        r["umi"][d] = (r["umi"][a] & ~np.uint32(31)) | rng.integers(0, 32, length, dtype=np.uint32)
        shift += length - 1
    return r


def _assert_runs_straddle_tiles(res, r, canon_sorted, big_run):
    """every length class of the repair step holds a run that lies across a multiple of the run-length tile"""
    reads, cols = _sorted_key_columns(res, r, canon_sorted)
    tile = _rl_tile(len(reads))
    starts, ends = _runs_above_low_bits(cols, UMI_LOW)
    length = ends - starts
    across = (starts // tile) != ((ends - 1) // tile)
    mixed = np.array([((np.diff(cols[3][s:e]) == 0) & (np.diff(cols[4][s:e]) != 0)).any() if e - s > 1 else False
                      for s, e in zip(starts, ends)])
    for lo, hi in ((2, 12), (13, 64), (65, 4096), (4097, 65536)):
        cls = (length >= lo) & (length <= hi)
        assert (cls & across).any(), "no run of %d..%d keys lies across a multiple of %d" % (lo, hi, tile)
        assert (cls & mixed).any(), "no run of %d..%d keys holds one UMI with both UmiTypes" % (lo, hi)
    if big_run <= 65536:
        big = np.argmax(length)
        assert length[big] >= big_run * 0.9 and (ends[big] - 1) // tile - starts[big] // tile >= 3
    return tile


@pytest.mark.parametrize("big_run,wide", [(50_000, False), (90_000, False), (50_000, True)])
def test_run_heads_counted_by_the_finishing_step(big_run, wide):
    """Runs of keys that agree above their low 6 bits, out of order when the sort on the top bits leaves them: 2 - 12 keys
    (ordered in registers), 13 - 64 (by a wave), 65 - 4096 (by a workgroup in LDS), more (one lane through memory), one of
    each laid across a multiple of the run-length tile, and one of 50 000 keys that crosses several tiles; UmiTypes mixed,
    so that keys equal above bit 0 occur inside the runs.  The run-length pass takes its tile counts from the finishing
    step (CRGPU_STAT_RL_COUNTS_FROM_FINISH) -- a wrong count leaves gaps or overlaps in the distinct keys and nothing
    downstream survives that: every DupInfo field, the matrix and the molecule table equal the oracle's.  A run of 90 000
    keys is too long for the repair: the buffer is sorted again on all bits (CRGPU_STAT_SORT_REFINISHED) and the counts
    come from the count pass, with the same result.  wide: 64-bit keys, ten low bits left to the finishing step."""
    from test_gpu_count import _compare_with_oracle, _needs_onesweep

    _needs_onesweep()
    import gpu_helpers as G
    from cellranger_amd import synth as S

    n = 260_000
    w = S.Workload(n_total=n, seed=31, n_wl=6_794_880 if wide else 2000, n_cells=40, n_ambient=200, n_genes=40, umi_len=12, umi_err=0.0,
                   cb_err=0.01, n_rate=0.001, no_feature_frac=0.05, reads_per_umi=1)
    c = G.fresh_ctx(dense=False)   # the positions this test plants belong to the whitelist-rank layout
    c.set_whitelist(0, w.wl_packed, length=16)
    _, canon_sorted = c.canon_order()
    r = _heads_inputs(w, big_run, canon_sorted)
    from_finish0 = c.stat(STAT_RL_COUNTS_FROM_FINISH)
    res, m = _compare_with_oracle(c, w, r, n, 36_601 if wide else 40)
    _assert_runs_straddle_tiles(res, r, canon_sorted, big_run)
    assert m.nnz > 1000
    if big_run > 65_536:
        assert c.stat(STAT_SORT_REFINISHED) > 0 and c.stat(STAT_RL_COUNTS_FROM_FINISH) == from_finish0
    else:
        assert c.stat(STAT_SORT_REFINISHED) == 0 and c.stat(STAT_RL_COUNTS_FROM_FINISH) > from_finish0
    c.close()


# ---- per-key state across calls -----------------------------------------------------------------------------------------------------
def _state_case(kind):
    """(workload, reads, n_features, n_libs, mux_mask, on_target or None)"""
    from cellranger_amd import synth as S
    from cellranger_amd._lib import FLAG_NONTXOMIC

    if kind == "dense":
        # tiny UMI space, few features, three libraries (one without UMI correction): dense Hamming-1 neighbourhoods, many
        # sources per target, tied counts, targets that are corrected away themselves
        n = 120_000
        w = S.Workload(n_total=n, seed=12, n_wl=2000, n_cells=40, n_ambient=500, n_genes=7, umi_len=5, umi_err=0.05, cb_err=0.01,
                       n_rate=0.002, no_feature_frac=0.1, reads_per_umi=2, n_libs=3)
        r = w.host_reads(0, n)
        rng = np.random.default_rng(12)
        r["flags"] = (r["flags"] | np.where(rng.random(n) < 0.3, FLAG_NONTXOMIC, 0)).astype(np.uint8)
        return w, r, 7, 3, 0b100, None
    if kind == "giant":
        # three barcodes, two features, 65 536 UMIs: segments of far more than UE_CAP = 4096 distinct keys (the giant chain),
        # every one of them across many UMI tile edges
        n = 150_000
        w = S.Workload(n_total=n, seed=21, n_wl=100, n_cells=3, n_ambient=0, n_genes=2, umi_len=8, umi_err=0.02, cb_err=0.0,
                       n_rate=0.0, no_feature_frac=0.0, reads_per_umi=3, sigma=0.1)
        return w, w.host_reads(0, n), 2, 1, 0, None
    if kind == "targeted":
        # half of the features on target, threshold 3: the filter reads the final read count of every corrected key
        n = 200_000
        w = S.Workload(n_total=n, seed=S.SEED0 + 11, n_wl=50_000, n_cells=200, n_ambient=5000, n_genes=600, umi_len=7, umi_err=0.03,
                       reads_per_umi=3)
        return w, w.host_reads(0, n), 600, 1, 0, (np.arange(600) % 2 == 0).astype(np.uint8)
    raise ValueError(kind)


def _complement_umis(r, umi_len):
    """every UMI base complemented: the same reads stay valid (a homopolymer stays one, the N flags live in the quality
    bytes), Hamming distances survive, the order of the UMIs inside every segment is reversed"""
    r2 = {k: v.copy() for k, v in r.items()}
    r2["umi"] = (r["umi"] ^ np.uint32((1 << (2 * umi_len)) - 1)).astype(np.uint32)
    return r2


def _distinct_keys(res, r):
    """distinct (barcode, feature, library, UMI) among the reads the oracle hands to the count stage"""
    has = res.dupinfo["has_dupinfo"] != 0
    rows = np.concatenate([res.corrected_cb[has].astype(np.int64), r["feature"][has].astype(np.int64)[:, None],
                           (r["flags"][has] & 0x0F).astype(np.int64)[:, None], r["umi"][has].astype(np.int64)[:, None]], 1)
    return len(np.unique(rows, axis=0))


@pytest.mark.parametrize("overlap", [None, "0", "2"])
@pytest.mark.parametrize("kind", ["dense", "giant", "targeted"])
def test_second_call_in_one_context_reads_no_stale_state(kind, overlap, monkeypatch):
    """The context's pool hands a request a free block of exactly the same size, so two calls with the same number of keys
    and of distinct keys in ONE context give the second call the first call's state arrays: (a) the same input twice -- state
    that is not initialised again shows as doubled read counts; (b) the input with every UMI base complemented after the
    input itself -- the same block sizes, the targets elsewhere, so a reader of corr / inc_all / minidx that does not ask the
    state word first sees the first call's values.  The SECOND call is compared with the oracle: every field of the
    per-read DupInfo (count_records), the keys-only path (count_keys), matrix, molecule table, summary; with the
    targeted-panel filter on and off; on one stream (CRGPU_DEDUP_OVERLAP=0), with the second stream for every input size
    (=2), and as by default."""
    from test_gpu_count import _compare_with_oracle, _run_gpu

    import gpu_helpers as G
    import oracle_lib as O

    if overlap is not None:
        monkeypatch.setenv("CRGPU_DEDUP_OVERLAP", overlap)
    w, r1, n_features, n_libs, mux_mask, on_target = _state_case(kind)
    n = w.n_total
    r2 = _complement_umis(r1, w.umi_len)
    for first, second in ((r1, r1), (r1, r2)):
        c = G.fresh_ctx()
        for lib in range(n_libs):
            c.set_whitelist(lib, w.wl_packed, length=16)
        try:
            if on_target is not None:
                c.set_target_filter(on_target, 3)
                O.set_target_filter(on_target, 3)
            _run_gpu(c, first, n, w.cb_len, w.umi_len, n_features, n_libs, mux_mask)
            c.reset_counts()
            res, m = _compare_with_oracle(c, w, second, n, n_features, n_libs=n_libs, mux_mask=mux_mask)
            assert m.nnz > 0 and int((res.dupinfo["is_corrected"] != 0).sum()) > 100
            if second is not first:
                res1 = _oracle(w, first, n_lib=n_libs, multiplexing_lib_mask=mux_mask)
                assert _distinct_keys(res1, first) == _distinct_keys(res, second)
                assert int((res1.dupinfo["has_dupinfo"] != 0).sum()) == int((res.dupinfo["has_dupinfo"] != 0).sum())
            if on_target is not None:
                assert int((res.dupinfo["is_filtered_target"] != 0).sum()) > 1000
        finally:
            O.set_target_filter(None)
        if on_target is not None:   # and with the filter off again, on the blocks the filtered calls used
            c.set_target_filter(None)
            c.reset_counts()
            res3, m3 = _compare_with_oracle(c, w, second, n, n_features, n_libs=n_libs, mux_mask=mux_mask)
            assert int((res3.dupinfo["is_filtered_target"] != 0).sum()) == 0 and m3.data.sum() > m.data.sum()
        c.close()
