"""GPU parity tests of the probe x barcode counts of a Flex / RTL well: BcUmiInfo::probe_counts (cr_types/src/types.rs:190-204)
as ProbeBarcodeCount triplets (types.rs:141-146), the raw probe matrix (cr_lib/src/probe_barcode_matrix.rs:176-262) and the
two sums of collate_probe_metrics (cr_lib/src/gdna_utils.rs:217-237).

The expected values come from the oracle alone: the reads it marks is_umi_count are the molecules' representative reads,
their barcode is the oracle's corrected barcode, their probe the probe handed in per read; triplets = np.unique with counts
over (barcode rank, probe) of those reads with a probe.  Matrix and metrics are numpy restatements over those triplets.
Everything is compared for equality."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
MISS = 0xFFFFFFFF
NO_FEATURE = 0xFFFFFFFF
STAT_WAVE, STAT_WORKGROUP, STAT_GLOBAL = 12, 13, 14
ERANGE, ESTATE, EINVAL = -6, -5, -1
LDS_CAP = 32768   # the largest segment the LDS classes take by default
N_1M = 1_000_000


# ---- inputs -----------------------------------------------------------------------------------------------------------------
def _workload(kind):
    from cellranger_amd import synth as S

    n_libs = 2 if kind == "two_libs" else 1
    return S.Workload(n_total=N_1M, seed=S.SEED0 + 3, n_cells=300, n_ambient=20000, n_libs=n_libs), n_libs


@functools.lru_cache(maxsize=None)
def _case(kind):
    """the 1 M-read cfg3-shaped input of the count tests (one / two libraries; `giants`: three barcodes -- whitelist rank 0, the
    last rank, one in the middle -- get 48 000 reads each with distinct random UMIs) and the oracle's run over it"""
    import gpu_helpers as G
    import oracle_lib as O
    from cellranger_amd import engine as E

    w, n_libs = _workload(kind)
    n = N_1M
    r = w.host_reads(0, n)
    canon_sorted = np.sort(w.wl_packed)
    giants = []
    if kind == "giants":
        rng = np.random.default_rng(5)
        sel = rng.permutation(n)[:3 * 48_000].reshape(3, 48_000)
        giants = [0, len(canon_sorted) - 1, len(canon_sorted) // 2]
        for rank, rows in zip(giants, sel):
            r["cb"][rows] = canon_sorted[rank]
            r["cb_qualn"][rows] &= 0x7F          # no N in the barcode
            r["flags"][rows] &= 0xEF             # FLAG_CB_HAS_N
            r["umi"][rows] = rng.permutation(1 << 24)[:len(rows)].astype(np.uint32)
            r["umi_qualn"][rows] &= 0x7F
    wl = O.Whitelist(E.unpack_seqs(w.wl_packed, w.cb_len))
    res = O.run_pipeline(G.oracle_reads_from_packed(r, w.cb_len, w.umi_len), [wl] * n_libs, n_lib=n_libs, n_threads=4,
                         want_dupinfo=True)
    _, exp_b = G.oracle_expected_idx(res, canon_sorted)
    rep = np.flatnonzero(res.dupinfo["is_umi_count"] != 0)     # the representative read of every molecule
    return dict(w=w, n_libs=n_libs, r=r, canon_sorted=canon_sorted, rep=rep, rep_bc=exp_b[rep], giants=giants)


def _probes(kind, feature, n_genes):
    """probe index per read.  hash: of (feature, read ordinal), not monotone in the feature, a few per feature so that
    molecules share probes, some reads without a probe; asc / desc: ascending / strictly descending with the feature"""
    n = len(feature)
    f = feature.astype(np.uint64)
    if kind == "hash":
        n_probes = 40_000
        h = (f * np.uint64(2654435761) + (np.arange(n, dtype=np.uint64) % np.uint64(7)) * np.uint64(40503)) >> np.uint64(5)
        p = (h % np.uint64(n_probes + 1)).astype(np.int64) - 1
    elif kind == "asc":
        n_probes, p = n_genes, f.astype(np.int64)
    else:
        n_probes, p = n_genes, np.int64(n_genes - 1) - f.astype(np.int64)
    p[feature == NO_FEATURE] = -1
    return p.astype(np.int32), n_probes


def _expected_triplets(case, probe):
    p = probe[case["rep"]].astype(np.int64)
    keep = p >= 0
    key = (case["rep_bc"][keep].astype(np.uint64) << np.uint64(32)) | p[keep].astype(np.uint64)
    uniq, cnt = np.unique(key, return_counts=True)
    return (uniq >> np.uint64(32)).astype(np.uint32), (uniq & np.uint64(0xFFFFFFFF)).astype(np.uint32), cnt.astype(np.uint32)


def _expected_matrix(trip, sample_ranks):
    ebc, epr, ect = trip
    lo, hi = np.searchsorted(ebc, sample_ranks, "left"), np.searchsorted(ebc, sample_ranks, "right")
    indptr = np.concatenate([[0], np.cumsum(hi - lo)]).astype(np.int64)
    take = np.concatenate([np.arange(a, b) for a, b in zip(lo, hi)] + [np.zeros(0, np.int64)]).astype(np.int64)
    return indptr, epr[take].astype(np.int32), ect[take].astype(np.int32)


def _expected_metrics(trip, n_probes, cell_ranks):
    ebc, epr, ect = trip
    all_, filt = np.zeros(n_probes, np.uint64), np.zeros(n_probes, np.uint64)
    np.add.at(all_, epr, ect.astype(np.uint64))
    in_cells = np.isin(ebc, cell_ranks)
    np.add.at(filt, epr[in_cells], ect[in_cells].astype(np.uint64))
    return all_, filt


def _out_of_feature_order(case, probe):
    """barcodes whose molecules, in (feature) order, do not carry ascending probes"""
    rep, bc = case["rep"], case["rep_bc"]
    order = np.lexsort((case["r"]["feature"][rep], bc))
    b, p = bc[order], probe[rep][order].astype(np.int64)
    p = np.where(p < 0, np.int64(1) << 40, p)   # no probe: after every probe
    bad = (b[1:] == b[:-1]) & (p[1:] < p[:-1])
    return len(np.unique(b[1:][bad]))


# ---- GPU side ---------------------------------------------------------------------------------------------------------------
def _ctx(monkeypatch, cap, dense=None):
    import gpu_helpers as G

    if cap is None:
        monkeypatch.delenv("CRGPU_PROBE_SEG_CAP", raising=False)
    else:
        monkeypatch.setenv("CRGPU_PROBE_SEG_CAP", str(cap))   # read when the context is created
    return G.fresh_ctx(dense=dense)


def _gpu_counts(c, case, probe):
    import gpu_helpers as G

    w, r, n = case["w"], case["r"], N_1M
    for lib in range(case["n_libs"]):
        c.set_whitelist(lib, w.wl_packed, length=16)
    _, canon_sorted = c.canon_order()
    assert np.array_equal(canon_sorted, case["canon_sorted"])
    _, _, _, dev = G.gpu_barcode_stage(c, r, n)
    c.set_key_layout(w.n_genes, w.umi_len, case["n_libs"], 0)
    d = [c.upload(r["umi"]), c.upload(r["umi_qualn"]), c.upload(r["feature"]), c.upload(probe)]
    recs = c.records(n, w.umi_len, dev["idx"], d[0], d[1], d[2], dev["flags"], d_probe_idx=d[3])
    counts = c.count_records(recs)
    c.synchronize()
    return counts, (dev, d)


def _routes(c):
    return c.stat(STAT_WAVE), c.stat(STAT_WORKGROUP), c.stat(STAT_GLOBAL)


def _check_everything(c, counts, case, probe, n_probes, cap):
    exp = _expected_triplets(case, probe)
    ebc, epr, ect = exp
    assert len(ebc) > 10_000 and ect.max() > 1                       # not vacuous
    bc, pr, ct = counts.probe_triplets(n_probes)
    assert np.array_equal(bc, ebc) and np.array_equal(pr, epr) and np.array_equal(ct, ect)
    # the route every segment took: one segment per barcode with a molecule
    wave, wg, glob = _routes(c)
    n_segments = len(np.unique(case["rep_bc"]))
    assert wave + wg + glob == n_segments
    sizes = np.bincount(np.unique(case["rep_bc"], return_inverse=True)[1])
    eff = LDS_CAP if cap is None else min(cap, LDS_CAP)
    assert glob == int((sizes > eff).sum())
    assert wave == int((sizes <= min(eff, 64)).sum()) and wg == int(((sizes > 64) & (sizes <= eff)).sum())
    # device views hold the same arrays; a second computation (another n_probes forces one) gives the same bytes
    d_bc, d_pr, d_ct, nt = counts.probe_triplets_dev(n_probes)
    assert nt == len(ebc)
    from cellranger_amd import _lib
    for d_view, want in ((d_bc, ebc), (d_pr, epr), (d_ct, ect)):   # library-owned views: copied, never freed here
        got = np.zeros(nt, np.uint32)
        c._check(c.L.crgpu_memcpy_d2h(c.h, _lib.ptr(got), d_view, nt * 4))
        assert np.array_equal(got, want)
    again = counts.probe_triplets(n_probes + 1)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(again, (bc, pr, ct)))
    # the property of case 9: per barcode the counts add up to its molecules with a probe (crgpu_counts_probe_idx)
    mol_bc, mol_probe = counts.molecules()["bc"], counts.probe_idx()
    assert np.array_equal(np.bincount(bc, weights=ct, minlength=len(case["canon_sorted"])).astype(np.int64),
                          np.bincount(mol_bc[mol_probe >= 0], minlength=len(case["canon_sorted"])))
    return exp


@pytest.mark.parametrize("cap", [None, 0, 1000])
@pytest.mark.parametrize("kind,probes", [("one_lib", "hash"), ("two_libs", "hash"), ("one_lib", "asc"), ("one_lib", "desc"),
                                         ("giants", "hash"), ("giants", "asc"), ("giants", "desc")])
def test_probe_triplets_match_the_oracle(kind, probes, cap, monkeypatch):
    """cases 1-4: hashed / ascending / descending probes, one and two libraries (pooled), planted giants at rank 0, the last
    rank and in the middle; default routes, every segment through the global sort (cap 0), and a cap of 1000 molecules that
    sends segments to the wave class, the workgroup class and the sort"""
    case = _case(kind)
    probe, n_probes = _probes(probes, case["r"]["feature"], case["w"].n_genes)
    disorder = _out_of_feature_order(case, probe)
    assert disorder == 0 if probes == "asc" else disorder > 100
    c = _ctx(monkeypatch, cap)
    counts, keep = _gpu_counts(c, case, probe)
    ebc, _, _ = _check_everything(c, counts, case, probe, n_probes, cap)
    wave, wg, glob = _routes(c)
    if cap == 0:
        assert wave == 0 and wg == 0 and glob > 10_000
    elif cap == 1000:
        assert wave > 1000 and wg >= 1 and glob >= 1     # every class is taken
    else:
        assert wave > 1000 and wg > 100
        assert glob == (3 if kind == "giants" else 0)
    if kind == "giants":   # the segment edges: the first and the last barcode rank carry a giant
        assert ebc[0] == 0 and ebc[-1] == len(case["canon_sorted"]) - 1
    counts.free()
    c.close()


@pytest.mark.parametrize("dense", [True, False])
def test_probe_triplets_with_dense_and_rank_barcode_keys(dense, monkeypatch):
    """case 5: the barcode field of the molecule keys holds BarcodeIndex columns (dense) or whitelist ranks; the triplets
    carry whitelist ranks either way"""
    case = _case("giants")
    probe, n_probes = _probes("hash", case["r"]["feature"], case["w"].n_genes)
    c = _ctx(monkeypatch, None, dense=dense)
    counts, keep = _gpu_counts(c, case, probe)
    _check_everything(c, counts, case, probe, n_probes, None)
    counts.free()
    c.close()


def test_probe_matrix_and_metrics_match_numpy_over_the_oracle_triplets(monkeypatch):
    """case 7 + the metrics: the matrix over the context's BarcodeIndex, over a sample list that omits observed barcodes and
    lists barcodes without probe counts (inside and outside the BarcodeIndex); select_barcodes_dev of the full matrix at the
    sample's positions equals the directly assembled sample matrix; sum_matrices_dev works on it"""
    case = _case("two_libs")
    probe, n_probes = _probes("hash", case["r"]["feature"], case["w"].n_genes)
    c = _ctx(monkeypatch, None)
    counts, keep = _gpu_counts(c, case, probe)
    exp = _expected_triplets(case, probe)
    ebc = exp[0]
    # full matrix: the columns of the feature matrix
    bcf, ftf, ctf = counts.triplets_dev()
    feat_rank = c.assemble_matrix_dev(bcf, ftf, ctf, counts.n_triplets).download()[0]
    full = counts.probe_matrix(n_probes)
    rank, indptr, indices, data = full.download()
    assert np.array_equal(rank, feat_rank)
    e_indptr, e_indices, e_data = _expected_matrix(exp, rank)
    assert e_indptr[-1] == len(ebc) > 10_000      # every observed barcode is a column of the BarcodeIndex
    assert np.array_equal(indptr, e_indptr) and np.array_equal(indices, e_indices) and np.array_equal(data, e_data)
    empty_cols = rank[np.diff(indptr) == 0]
    assert len(empty_cols) > 10                    # barcodes with reads but without a probed molecule
    # a sample: every other observed barcode + some columns without probe counts
    observed = np.unique(ebc)
    sample = np.unique(np.concatenate([observed[::2], empty_cols[:50]])).astype(np.uint32)
    sm = counts.probe_matrix(n_probes, sample)
    s_rank, s_indptr, s_indices, s_data = sm.download()
    x_indptr, x_indices, x_data = _expected_matrix(exp, sample)
    assert np.array_equal(s_rank, sample) and 0 < x_indptr[-1] < len(ebc)
    assert np.array_equal(s_indptr, x_indptr) and np.array_equal(s_indices, x_indices) and np.array_equal(s_data, x_data)
    sel = c.select_barcodes_dev(full, np.searchsorted(rank, sample).astype(np.uint64))
    for a, b in zip(sel.download(), (s_rank, s_indptr, s_indices, s_data)):
        assert np.array_equal(a, b)
    twice = c.sum_matrices_dev(sm, sel).download()
    assert np.array_equal(twice[1], s_indptr) and np.array_equal(twice[2], s_indices) and np.array_equal(twice[3], 2 * s_data)
    # ranks outside the BarcodeIndex are empty columns, too
    outside = np.setdiff1d(np.arange(len(case["canon_sorted"]), dtype=np.uint32), rank)[:20]
    mixed = np.unique(np.concatenate([observed[1::3], outside])).astype(np.uint32)
    m_rank, m_indptr, m_indices, m_data = counts.probe_matrix(n_probes, mixed).download()
    y_indptr, y_indices, y_data = _expected_matrix(exp, mixed)
    assert np.array_equal(m_rank, mixed)
    assert np.array_equal(m_indptr, y_indptr) and np.array_equal(m_indices, y_indices) and np.array_equal(m_data, y_data)
    # an empty sample: no column
    z = counts.probe_matrix(n_probes, np.zeros(0, np.uint32))
    assert z.n_barcodes == 0 and z.nnz == 0 and np.array_equal(z.download()[1], [0])
    # metrics: the cells = the 300 barcodes with most molecules
    sizes = np.bincount(case["rep_bc"], minlength=len(case["canon_sorted"]))
    cells = np.sort(np.argsort(sizes)[-300:]).astype(np.uint32)
    all_, filt = counts.probe_metrics(n_probes, cells)
    e_all, e_filt = _expected_metrics(exp, n_probes, cells)
    assert np.array_equal(all_, e_all) and np.array_equal(filt, e_filt)
    assert 0 < filt.sum() < all_.sum() == exp[2].sum()
    none_all, none_filt = counts.probe_metrics(n_probes, np.zeros(0, np.uint32))
    assert np.array_equal(none_all, e_all) and not none_filt.any()
    # unsorted lists are refused
    from cellranger_amd import engine as E
    for bad in (sample[::-1].copy(), np.array([5, 5], np.uint32)):
        with pytest.raises(E.CrgpuError, match="strictly ascending") as ei:
            counts.probe_matrix(n_probes, bad)
        assert ei.value.code == EINVAL
        with pytest.raises(E.CrgpuError, match="strictly ascending") as ei:
            counts.probe_metrics(n_probes, bad)
        assert ei.value.code == EINVAL
    counts.free()
    c.close()


def test_no_probes_bad_probes_and_counts_without_probes(monkeypatch):
    """case 6"""
    import gpu_helpers as G
    from cellranger_amd import engine as E
    from cellranger_amd import synth as S

    n = 60_000
    w = S.Workload(n_total=n, seed=9, n_wl=3000, n_cells=40, n_ambient=400, n_genes=50)
    r = w.host_reads(0, n)
    for cap in (None, 0):
        c = _ctx(monkeypatch, cap)
        c.set_whitelist(0, w.wl_packed, length=16)
        _, _, _, dev = G.gpu_barcode_stage(c, r, n)
        c.set_key_layout(w.n_genes, w.umi_len, 1, 0)
        d_umi, d_uq, d_ft = c.upload(r["umi"]), c.upload(r["umi_qualn"]), c.upload(r["feature"])

        def counts_with(probe):
            d_p = c.upload(probe)
            out = c.count_records(c.records(n, w.umi_len, dev["idx"], d_umi, d_uq, d_ft, dev["flags"], d_probe_idx=d_p))
            c.synchronize()
            return out

        # every read without a probe: zero triplets, empty columns, zero metrics
        none = counts_with(np.full(n, -1, np.int32))
        assert none.n_molecules > 1000
        assert all(len(a) == 0 for a in none.probe_triplets(10))
        assert none.probe_triplets_dev(10)[3] == 0
        rank, indptr, indices, data = none.probe_matrix(10).download()
        assert len(rank) > 40 and not indptr.any() and len(indices) == 0 and len(data) == 0
        a, f = none.probe_metrics(10, rank[:5])
        assert len(a) == 10 and not a.any() and not f.any()
        # one molecule with probe == n_probes / with probe -2: CRGPU_ERANGE (the same probes are fine for a larger set)
        probe = (np.arange(n) % 10).astype(np.int32)
        ok = counts_with(probe)
        assert len(ok.probe_triplets(10)[0]) > 100
        with pytest.raises(E.CrgpuError, match="probe index outside") as ei:
            ok.probe_triplets(9)
        assert ei.value.code == ERANGE
        with pytest.raises(E.CrgpuError, match="probe index outside") as ei:
            ok.probe_matrix(9)
        assert ei.value.code == ERANGE
        assert len(ok.probe_triplets(10)[0]) > 100          # the counts stay usable
        low = counts_with(np.where(np.arange(n) % 10 == 3, -2, probe).astype(np.int32))
        with pytest.raises(E.CrgpuError, match="probe index outside") as ei:
            low.probe_triplets(10)
        assert ei.value.code == ERANGE
        # counts made from keys, or from records without probes: CRGPU_ESTATE
        recs = c.records(n, w.umi_len, dev["idx"], d_umi, d_uq, d_ft, dev["flags"])
        d_keys = c.empty(n, np.uint64)
        from_keys = c.count_keys(d_keys, c.build_keys(recs, d_keys))
        without = c.count_records(recs)
        for bad in (from_keys, without):
            for call in (lambda: bad.probe_triplets(10), lambda: bad.probe_triplets_dev(10), lambda: bad.probe_matrix(10),
                         lambda: bad.probe_metrics(10, rank[:5])):
                with pytest.raises(E.CrgpuError, match="without crgpu_records.d_probe_idx") as ei:
                    call()
                assert ei.value.code == ESTATE
        # no molecules at all: zero triplets, not an error
        recs0 = c.records(0, w.umi_len, dev["idx"], d_umi, d_uq, d_ft, dev["flags"], d_probe_idx=c.upload(probe))
        zero = c.count_records(recs0)
        assert zero.n_molecules == 0 and len(zero.probe_triplets(10)[0]) == 0
        c.close()


# ---- case 8: a 24-base GelBeadAndProbe well (built as tests/test_gpu_segments.py builds its own) -----------------------------
def _mutate(rng, seqs, p_sub, p_n):
    acgt = np.frombuffer(b"ACGT", np.uint8)
    s = seqs.copy()
    n, L = s.shape
    sub = rng.random(n) < p_sub
    pos = rng.integers(0, L, n)
    s[sub, pos[sub]] = acgt[rng.integers(0, 4, int(sub.sum()))]
    nn = rng.random(n) < p_n
    pos = rng.integers(0, L, n)
    s[nn, pos[nn]] = ord("N")
    return s


def _segment_stage(c, rows_s, rows_q, n, stride, offset, length):
    d_rs, d_rq = c.upload(rows_s), c.upload(rows_q)
    d_pk, d_qn, d_fl = c.empty(n, np.uint32), c.empty((n, length), np.uint8), c.zeros(n, np.uint8)
    c.pack_rows(d_rs, d_rq, n, stride, offset, length, d_pk, d_qn, d_fl)
    d_idx = c.empty(n, np.uint32)
    c.match_and_count(d_pk, d_fl, n, d_idx)
    d_idx_a = c.empty(n, np.uint32)
    d_idx_a.upload(d_idx.to_host())
    c.correct(d_pk, d_qn, d_fl, n, d_idx)
    c.synchronize()
    return d_idx_a, d_idx


@pytest.mark.parametrize("big", [False, True])
def test_gel_bead_and_probe_well(big, monkeypatch):
    """gel bead 16 + probe barcode 8 bases, corrected segment by segment; the probe INDEX of a read (the probe its insert maps
    to) is independent of its probe-barcode segment.  big: 737 280 x 16 barcodes, which need dense barcode keys."""
    import gpu_helpers as G
    import oracle_lib as O
    from cellranger_amd import engine as E

    rng = np.random.default_rng(4)
    LA, LB, LU = 16, 8, 12
    n_pb = 16
    n_gb, n_feat, n = (737_280, 36_601, 80_000) if big else (3000, 60, 80_000)
    wl_a = np.unique(rng.integers(0, 1 << 32, n_gb * 2, dtype=np.uint64).astype(np.uint32))[:n_gb]
    wl_b = np.unique(rng.integers(0, 1 << 16, n_pb * 8, dtype=np.uint64).astype(np.uint32))
    wl_b = np.sort(rng.permutation(wl_b)[:n_pb])
    a_ascii, b_ascii = E.unpack_seqs(wl_a, LA), E.unpack_seqs(wl_b, LB)
    cells = rng.integers(0, n_gb, 400)
    cell = cells[np.minimum(rng.zipf(1.3, n) - 1, 399)]
    pb = rng.integers(0, n_pb, n)
    gene = np.minimum(rng.zipf(1.5, n) - 1, n_feat - 1).astype(np.uint32)
    gene[rng.random(n) < 0.03] = MISS
    n_probes = 3 * n_feat
    probe = ((gene.astype(np.int64) * 7919 + rng.integers(0, 3, n)) % n_probes).astype(np.int32)
    probe[rng.random(n) < 0.1] = -1
    umi_pk = rng.integers(0, 1 << 24, n, dtype=np.uint64).astype(np.uint32)
    umi_ascii = E.unpack_seqs(umi_pk, LU)
    seg_a, seg_b = _mutate(rng, a_ascii[cell], 0.08, 0.01), _mutate(rng, b_ascii[pb], 0.08, 0.01)
    stride = LA + LU + LB
    rows_s = np.hstack([seg_a, umi_ascii, seg_b])
    rows_q = rng.integers(35, 74, (n, stride)).astype(np.uint8)

    monkeypatch.delenv("CRGPU_PROBE_SEG_CAP", raising=False)
    ca, cb, cc = G.fresh_ctx(), G.fresh_ctx(), G.fresh_ctx(dense=True if big else None)
    ca.set_whitelist(0, wl_a, length=LA)
    cb.set_whitelist(0, wl_b, length=LB)
    _, a_sorted = ca.canon_order()
    _, b_sorted = cb.canon_order()
    cc.set_barcode_segments(0, [a_sorted, b_sorted], [LA, LB])
    da_a, da = _segment_stage(ca, rows_s, rows_q, n, stride, 0, LA)
    db_a, db = _segment_stage(cb, rows_s, rows_q, n, stride, LA + LU, LB)
    d_idx = cc.empty(n, np.uint32)
    cc.combine_segments(0, [da_a, db_a], n, d_idx)                         # after the exact match: VALID
    cc.combine_segments(0, [da, db], n, d_idx, after_correction=True)      # after correction: CORRECTED
    idx_b = d_idx.to_host()
    d_rs, d_rq = cc.upload(rows_s), cc.upload(rows_q)
    d_um, d_uq = cc.empty(n, np.uint32), cc.empty((n, LU), np.uint8)
    cc.pack_rows(d_rs, d_rq, n, stride, LA, LU, d_um, d_uq)
    d_ft, d_fl, d_pr = cc.upload(gene), cc.zeros(n, np.uint8), cc.upload(probe)
    cc.set_key_layout(n_feat, LU, 1, 0)
    counts = cc.count_records(cc.records(n, LU, d_idx, d_um, d_uq, d_ft, d_fl, d_probe_idx=d_pr))
    bc, pr, ct = counts.probe_triplets(n_probes)

    # oracle: the barcode stage per segment, the count stage on the concatenated 24-base barcodes
    def seg_oracle(seqs, quals, wl_ascii):
        return O.run_pipeline(dict(cb=seqs, cb_qual=quals), [O.Whitelist(wl_ascii)], count=False)

    ra = seg_oracle(seg_a, rows_q[:, :LA], a_ascii)
    rb = seg_oracle(seg_b, rows_q[:, LA + LU:], b_ascii)
    _, exp_a = G.oracle_expected_idx(ra, a_sorted)
    _, exp_b = G.oracle_expected_idx(rb, b_sorted)
    valid_before = (ra.bc_state == 1) & (rb.bc_state == 1)
    valid_after = (ra.bc_state > 0) & (rb.bc_state > 0)
    want = np.full(n, MISS, np.uint32)
    want[valid_after] = exp_a[valid_after] * np.uint32(n_pb) + exp_b[valid_after]
    assert np.array_equal(idx_b, want)
    full = np.hstack([ra.corrected_cb, rb.corrected_cb])
    vh, ch = O.Hist(), O.Hist()
    for i in np.nonzero(valid_after)[0]:
        (vh if valid_before[i] else ch).observe_by(bytes(full[i]))
    reads = dict(cb=np.hstack([seg_a, seg_b]), cb_qual=np.hstack([rows_q[:, :LA], rows_q[:, LA + LU:]]), umi=umi_ascii,
                 umi_qual=rows_q[:, LA:LA + LU], feature=gene)
    res = O.run_pipeline(reads, [None], n_threads=4, want_dupinfo=True, bc_override=(full, valid_after.astype(np.uint8), vh, ch))
    rep = np.flatnonzero(res.dupinfo["is_umi_count"] != 0)
    ebc, epr, ect = _expected_triplets(dict(rep=rep, rep_bc=want[rep]), probe)
    assert len(ebc) > 1000 and ect.max() > 1
    assert _out_of_feature_order(dict(rep=rep, rep_bc=want[rep], r=dict(feature=gene)), probe) > 10
    assert np.array_equal(bc, ebc) and np.array_equal(pr, epr) and np.array_equal(ct, ect)
    # the probe matrix has the columns of the feature matrix of the well
    rank, indptr, indices, data = counts.probe_matrix(n_probes).download()
    t = counts.triplets()
    assert np.array_equal(rank, cc.assemble_matrix(t[0], t[1], t[2], n_feat).barcode_rank)
    e_indptr, e_indices, e_data = _expected_matrix((ebc, epr, ect), rank)
    assert np.array_equal(indptr, e_indptr) and np.array_equal(indices, e_indices) and np.array_equal(data, e_data)
    for c in (ca, cb, cc):
        c.close()


def test_probe_counts_add_up_at_20m_reads(monkeypatch):
    """case 9 at 20 M reads of the cfg3 model: per barcode the triplet counts sum to the molecules with a probe, the
    triplets are strictly ascending in (barcode, probe), and forcing every segment through the global sort changes nothing.
    (The oracle comparison is made at 1 M reads above.)"""
    from cellranger_amd import synth as S

    n = 20_000_000
    w = S.Workload(n_total=n, seed=S.SEED0 + 3)
    results = []
    for cap in (None, 0):
        c = _ctx(monkeypatch, cap)
        c.set_whitelist(0, w.wl_packed, length=16)
        c.set_key_layout(w.n_genes, w.umi_len, 1, 0)
        d = dict(cb=c.empty(n, np.uint32), cbq=c.empty((n, 16), np.uint8), fl=c.empty(n, np.uint8), umi=c.empty(n, np.uint32),
                 uq=c.empty((n, 12), np.uint8), ft=c.empty(n, np.uint32), idx=c.empty(n, np.uint32))
        c.synth(w, 0, n, cb=d["cb"].ptr, cb_qualn=d["cbq"].ptr, umi=d["umi"].ptr, umi_qualn=d["uq"].ptr, feature=d["ft"].ptr,
                flags=d["fl"].ptr)
        c.match_and_count(d["cb"], d["fl"], n, d["idx"])
        c.correct(d["cb"], d["cbq"], d["fl"], n, d["idx"])
        probe, n_probes = _probes("hash", d["ft"].to_host(), w.n_genes)
        d_pr = c.upload(probe)
        counts = c.count_records(c.records(n, w.umi_len, d["idx"], d["umi"], d["uq"], d["ft"], d["fl"], d_probe_idx=d_pr))
        bc, pr, ct = counts.probe_triplets(n_probes)
        wave, wg, glob = _routes(c)
        assert (wave == 0 and wg == 0 and glob > 100_000) if cap == 0 else (wave > 100_000 and wg > 1000)
        assert len(bc) > 1_000_000 and ct.max() > 1 and pr.max() < n_probes
        key = (bc.astype(np.uint64) << np.uint64(32)) | pr
        assert (key[1:] > key[:-1]).all()
        mol_bc, mol_probe = counts.molecules()["bc"], counts.probe_idx()
        assert np.array_equal(np.bincount(bc, weights=ct, minlength=w.n_wl).astype(np.int64),
                              np.bincount(mol_bc[mol_probe >= 0], minlength=w.n_wl))
        results.append((bc, pr, ct))
        counts.free()
        c.close()
    assert all(np.array_equal(a, b) for a, b in zip(*results))
