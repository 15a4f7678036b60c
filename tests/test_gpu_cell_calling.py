"""GPU parity tests of the initial cell call: column sums of the raw device matrix, the order-of-magnitude filter with its
bootstrap (crgpu_call_cells_ordmag_dev), the fixed cutoff, the called ranks and the filtered matrix.

The expected values come from tests/ordmag_numpy.py, a numpy restatement of lib/python/cellranger/cell_calling_helpers.py:832-964
(np.random.RandomState(0).choice, np.sort, np.searchsorted, a stable argsort, scipy.stats.norm.ppf).  Integers, the called
columns, the filtered CSC and the rounded confidence bounds are compared for equality; mean, variance, cv and the losses at a
relative 1e-12 (sums of 100 terms of a few ulp each stay below 1e-13)."""
import numpy as np
import pytest

import ordmag_numpy as R

pytestmark = pytest.mark.gpu
EINVAL, ERANGE = -1, -6
RTOL = 1e-12
N_1M = 1_000_000


# ---- inputs -----------------------------------------------------------------------------------------------------------------
def _profile(n_nonzero, seed):
    """UMI totals of a well: log-normal cells (2 % of the barcodes) over a geometric ambient tail, in random column order, with
    zero columns interleaved so that a barcode's place among the non-zero ones differs from its column"""
    rng = np.random.RandomState(seed)
    n_cells = max(1, n_nonzero // 50)
    vals = np.concatenate([np.round(rng.lognormal(8.5, 0.6, n_cells)), rng.geometric(0.15, n_nonzero)])[:n_nonzero]
    vals = np.maximum(vals, 1).astype(np.int64)
    rng.shuffle(vals)
    V = n_nonzero + n_nonzero // 3 + 2
    bc = np.zeros(V, np.int64)
    bc[np.sort(rng.choice(V, n_nonzero, replace=False))] = vals
    return bc


def _bounds_are_safe(ref):
    """the unrounded confidence bounds lie more than 1e-6 from a half-integer (NaN: the variance is 0, nothing is rounded)"""
    for k in ("lb_raw", "ub_raw"):
        x = ref[k]
        if not np.isnan(x) and abs(abs(x - np.floor(x)) - 0.5) <= 1e-6:
            return False
    return True


def _reference(make_counts, seed, **kw):
    """numpy's call on the first seed whose confidence bounds can be compared after rounding"""
    for s in range(seed, seed + 8):
        bc = make_counts(s)
        cols, ref = R.ordmag(bc, **kw)
        if _bounds_are_safe(ref):
            return bc, cols, ref
    raise AssertionError("no seed with safely rounded bounds")


# ---- comparison -------------------------------------------------------------------------------------------------------------
def _close(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.all(np.abs(a - b) <= RTOL * np.abs(b))


def _check_call(call, cols, ref):
    m = call.metrics
    print("n_nonzero %d recovered %d baseline %d filtered %d cutoff %s mean %.17g var %.17g lb %s ub %s" % (
        m["n_nonzero"], m["recovered_cells"], m["baseline_bc_idx"], m["filtered_bcs"], m["filtered_bcs_cutoff"],
        m["filtered_bcs_mean"], m["filtered_bcs_var"], m["filtered_bcs_lb"], m["filtered_bcs_ub"]))
    assert m["n_nonzero"] == ref["n_nonzero"]
    assert m["estimated"] == ref["estimated"]
    assert np.array_equal(m["recovered_boot"], ref["recovered_boot"])
    assert m["recovered_cells"] == ref["recovered_cells"]
    assert m["baseline_bc_idx"] == ref["baseline_bc_idx"]
    assert np.array_equal(m["top_n_boot"], ref["top_n_boot"])
    assert m["filtered_bcs"] == ref["filtered_bcs"] == call.n_cells
    assert m["filtered_bcs_cutoff"] == ref["cutoff"]          # None on both sides when the loop never set it
    assert np.array_equal(call.cols_host(), cols.astype(np.uint64))
    assert np.array_equal(m["filtered_bcs_lb"], ref["lb"], equal_nan=True) and np.array_equal(m["filtered_bcs_ub"], ref["ub"], equal_nan=True)
    assert _close(m["filtered_bcs_mean"], ref["mean"]) and _close(m["filtered_bcs_var"], ref["var"]) and _close(m["filtered_bcs_cv"], ref["cv"])
    assert _close(m["loss_boot"], ref["loss_boot"])


def _snapshot(call):
    """host copy of a call (outlives its context)"""
    return call.n_cells, call.cols_host(), dict(call.metrics)


def _same_call(a, b):
    """two snapshots agree bit for bit"""
    assert a[0] == b[0] and np.array_equal(a[1], b[1])
    assert a[2].keys() == b[2].keys()
    for k, v in a[2].items():
        w = b[2][k]
        if v is None or w is None:
            assert v is None and w is None, k
        else:
            assert np.array_equal(np.asarray(v, np.float64).view(np.uint64), np.asarray(w, np.float64).view(np.uint64)), k


# ---- the generator ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 12345])
def test_generator_kernel_is_numpys_raw_stream(seed):
    import gpu_helpers as G

    c = G.ctx()
    n = 3632 * 5 + 17                       # rounded down to whole chunks of the kernel
    d, ms = c.mt19937_stream(seed, n)
    got = d.to_host()
    assert len(got) == 3632 * 5 and ms > 0
    expect = np.random.RandomState(seed).randint(0, 1 << 32, len(got), dtype=np.uint64).astype(np.uint32)
    if seed == 0:
        assert list(expect[:2]) == [2357136044, 2546248239]
    assert np.array_equal(got, expect)


# ---- count vectors handed in directly ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("given", [False, True], ids=["estimate", "given"])
@pytest.mark.parametrize("n_nonzero", [1, 2, 49, 1000, 65_536, 65_537, 220_623, (1 << 20) + 3])
def test_count_vectors(n_nonzero, given):
    import gpu_helpers as G

    kw = dict(recovered_cells=max(60, n_nonzero // 30)) if given else dict(max_expected_cells=1 << 18)
    bc, cols, ref = _reference(lambda s: _profile(n_nonzero, s), 100 + n_nonzero % 97, **kw)
    assert ref["n_nonzero"] == n_nonzero and len(bc) > n_nonzero
    call = G.ctx().call_cells_ordmag(bc, **kw)
    _check_call(call, cols, ref)
    assert call.metrics["estimated"] != given


def test_all_zero_counts_and_no_columns():
    import gpu_helpers as G

    c = G.ctx()
    for bc in (np.zeros(1000, np.int64), np.zeros(0, np.int64)):
        for kw in (dict(), dict(recovered_cells=500), dict(force_cells=10)):
            call = c.call_cells_ordmag(bc, **kw)
            m = call.metrics
            assert call.n_cells == 0 and m["n_nonzero"] == 0 and m["filtered_bcs"] == 0 and m["filtered_bcs_cutoff"] is None
            assert m["recovered_cells"] == 0 and m["filtered_bcs_mean"] == 0 and m["filtered_bcs_var"] == 0 and m["filtered_bcs_lb"] == 0
            assert not m["top_n_boot"].any() and not m["recovered_boot"].any()
    cols, ref = R.ordmag(np.zeros(1000, np.int64))
    assert len(cols) == 0 and ref["filtered_bcs"] == 0
    # an all-zero well end to end: no called ranks, a filtered matrix without columns
    from cellranger_amd import synth as S

    w = S.Workload(n_total=1000, seed=3, n_wl=2000, n_cells=10, n_ambient=100, n_genes=20)
    cc = G.fresh_ctx()
    cc.set_whitelist(0, w.wl_packed, length=16)
    seen = np.zeros(cc.n_canon, np.uint32)
    seen[[5, 17, 900]] = 1                                   # three columns, no molecule in any of them
    cc.set_counts(0, 0, seen)
    z = np.zeros(0, np.uint32)
    raw = cc.assemble_matrix_dev(cc.upload(z), cc.upload(z), cc.upload(z), 0)
    assert raw.n_barcodes == 3 and raw.nnz == 0
    assert not cc.column_sums(raw).to_host().any()
    call = cc.call_cells_ordmag(raw)
    assert call.n_cells == 0 and len(call.cols_host()) == 0 and len(call.ranks) == 0
    f = call.filtered_matrix()
    assert f.n_barcodes == 0 and f.nnz == 0 and np.array_equal(f.download()[1], [0])
    cc.close()


def test_baseline_index_is_clamped_to_the_last_barcode():
    import gpu_helpers as G

    n = 49
    bc, cols, ref = _reference(lambda s: _profile(n, s), 7, recovered_cells=10_000)
    assert 10_000 * 0.01 >= n and ref["baseline_bc_idx"] == n - 1
    _check_call(G.ctx().call_cells_ordmag(bc, recovered_cells=10_000), cols, ref)


# ---- plateaus of equal counts at the cutoff ---------------------------------------------------------------------------------
def _plateau_counts(seed, ambient):
    """300 cells with distinct large totals, then `ambient`: a list of (value, how many) plateaus, in random column order"""
    rng = np.random.RandomState(seed)
    vals = np.concatenate([5000 + 7 * np.arange(300)] + [np.full(k, v) for v, k in ambient]).astype(np.int64)
    rng.shuffle(vals)
    V = len(vals) + 500
    bc = np.zeros(V, np.int64)
    bc[np.sort(rng.choice(V, len(vals), replace=False))] = vals
    return bc


def test_plateau_extending_by_less_than_a_fifth_is_taken_whole():
    import gpu_helpers as G

    # plateaus of 40 barcodes: whichever the cutoff lands in, it ends within 0.2 * nbcs (~60) places
    ambient = [(400 - 3 * i, 40) for i in range(100)]
    found = None
    for seed in range(40):
        bc = _plateau_counts(seed, ambient)
        cols, ref = R.ordmag(bc, recovered_cells=300)
        if not ref["gave_up"] and ref["filtered_bcs"] - ref["nbcs"] >= 3 and _bounds_are_safe(ref):
            found = (bc, cols, ref)
            break
    assert found, "no input whose cutoff lands inside a plateau"
    bc, cols, ref = found
    desc = np.sort(bc)[::-1]
    # the numpy side took the branch: the call grew over equal totals, and every barcode of the plateau is in
    assert ref["cutoff"] == desc[ref["nbcs"] - 1] and (bc[cols] >= ref["cutoff"]).sum() >= (bc == ref["cutoff"]).sum()
    assert set(np.flatnonzero(bc == ref["cutoff"])) <= set(cols)
    _check_call(G.ctx().call_cells_ordmag(bc, recovered_cells=300), cols, ref)


def test_plateau_extending_by_more_than_a_fifth_is_taken_in_part():
    import gpu_helpers as G

    ambient = [(30, 4000)]        # one plateau far longer than 0.2 * nbcs
    found = None
    for seed in range(40):
        bc = _plateau_counts(seed, ambient)
        cols, ref = R.ordmag(bc, recovered_cells=300)
        if ref["gave_up"] and ref["cutoff"] == 30 and _bounds_are_safe(ref):
            found = (bc, cols, ref)
            break
    assert found, "no input whose cutoff lands on the long plateau"
    bc, cols, ref = found
    # the numpy side took the branch: the loop gave up, what it had recorded stays, the plateau is cut
    on_plateau = np.flatnonzero(bc == 30)
    taken = np.intersect1d(cols, on_plateau)
    assert ref["filtered_bcs"] == ref["nbcs"] + int(0.2 * ref["nbcs"]) and 0 < len(taken) < len(on_plateau)
    assert np.array_equal(taken, on_plateau[-len(taken):])        # the larger columns win
    _check_call(G.ctx().call_cells_ordmag(bc, recovered_cells=300), cols, ref)


# ---- the fixed cutoff -------------------------------------------------------------------------------------------------------
def test_force_cells():
    import gpu_helpers as G

    c = G.ctx()
    bc = _profile(5000, 3)
    n = int((bc > 0).sum())
    desc = np.sort(bc)[::-1]
    through_ties = next(k for k in range(1500, n) if desc[k - 1] == desc[k] == desc[k - 2])   # cuts a run of equal totals
    for force in (100, through_ties, n - 1, n, n + 50, len(bc) + 10):
        cols, ref = R.fixed_cutoff(bc, force)
        call = c.call_cells_ordmag(bc, force_cells=force)
        m = call.metrics
        assert call.n_cells == m["filtered_bcs"] == ref["filtered_bcs"] == min(force, n)
        assert np.array_equal(call.cols_host(), cols.astype(np.uint64))
        assert m["filtered_bcs_cutoff"] == ref["cutoff"]
        assert (m["filtered_bcs_mean"], m["filtered_bcs_var"], m["filtered_bcs_cv"], m["filtered_bcs_lb"], m["filtered_bcs_ub"]) == (
            ref["mean"], 0.0, 0.0, ref["lb"], ref["ub"])
        assert not m["top_n_boot"].any() and not m["estimated"] and m["recovered_cells"] == 0
    ties = np.flatnonzero(bc == desc[through_ties])
    cols, _ = R.fixed_cutoff(bc, through_ties)
    taken = np.intersect1d(cols, ties)
    assert 0 < len(taken) < len(ties) and np.array_equal(taken, ties[-len(taken):])
    # no zero-count column behind the last non-zero one: the cutoff's place does not exist
    full = bc[bc > 0]
    assert c.call_cells_ordmag(full, force_cells=len(full)).metrics["filtered_bcs_cutoff"] is None


# ---- invariance -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_nonzero", [3000, 70_000])
def test_same_result_twice_and_with_small_batches(n_nonzero, monkeypatch):
    """70 000 barcodes: the estimate's 200 samples need two rounds of the generator, whose seam falls inside a batch"""
    import gpu_helpers as G

    bc, cols, ref = _reference(lambda s: _profile(n_nonzero, s), 11)
    monkeypatch.delenv("CRGPU_ORDMAG_BATCH", raising=False)
    c = G.fresh_ctx()
    call = c.call_cells_ordmag(bc)
    _check_call(call, cols, ref)
    first = _snapshot(call)
    _same_call(first, _snapshot(c.call_cells_ordmag(bc)))
    given = _snapshot(c.call_cells_ordmag(bc, recovered_cells=777))
    c.close()
    for batch in (1, 7):
        monkeypatch.setenv("CRGPU_ORDMAG_BATCH", str(batch))     # read when the context is created
        cb = G.fresh_ctx()
        _same_call(first, _snapshot(cb.call_cells_ordmag(bc)))
        _same_call(given, _snapshot(cb.call_cells_ordmag(bc, recovered_cells=777)))
        cb.close()


# ---- end to end -------------------------------------------------------------------------------------------------------------
def _csc_select(indptr, indices, data, cols):
    lens = np.diff(indptr)[cols]
    take = np.concatenate([np.arange(indptr[c], indptr[c + 1]) for c in cols] + [np.zeros(0, np.int64)]).astype(np.int64)
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), indices[take], data[take]


def test_end_to_end_from_reads_to_the_filtered_matrix():
    """the 1 M-read cfg3-shaped workload of the count tests through pass A / B and the count stage -> raw MatrixDev -> column
    sums (all features, and with a feature range masked out) -> the call (estimated and given) -> filtered matrix; the called
    ranks go into probe_metrics"""
    import gpu_helpers as G
    from cellranger_amd import engine as E
    from cellranger_amd import synth as S

    w = S.Workload(n_total=N_1M, seed=S.SEED0 + 3, n_cells=300, n_ambient=20000)
    r = w.host_reads(0, N_1M)
    probe = (r["feature"].astype(np.int64) % 977).astype(np.int32)
    probe[r["feature"] == 0xFFFFFFFF] = -1
    n_probes = 977
    c = G.fresh_ctx()
    c.set_whitelist(0, w.wl_packed, length=16)
    _, _, _, dev = G.gpu_barcode_stage(c, r, N_1M)
    c.set_key_layout(w.n_genes, w.umi_len, 1, 0)
    d = [c.upload(r["umi"]), c.upload(r["umi_qualn"]), c.upload(r["feature"]), c.upload(probe)]
    counts = c.count_records(c.records(N_1M, w.umi_len, dev["idx"], d[0], d[1], d[2], dev["flags"], d_probe_idx=d[3]))
    bcf, ftf, ctf = counts.triplets_dev()
    raw = c.assemble_matrix_dev(bcf, ftf, ctf, counts.n_triplets)
    rank, indptr, indices, data = raw.download()
    V = raw.n_barcodes
    assert V > 10_000 and raw.nnz > 100_000

    # column sums: all features, and without the features [n_genes / 4, n_genes / 2)
    col_of = np.repeat(np.arange(V), np.diff(indptr))
    all_sums = np.bincount(col_of, weights=data, minlength=V).astype(np.int64)
    assert np.array_equal(c.column_sums(raw).to_host(), all_sums.astype(np.uint32))
    mask = np.ones(w.n_genes, np.uint8)
    mask[w.n_genes // 4: w.n_genes // 2] = 0
    masked_sums = np.bincount(col_of, weights=data * mask[indices], minlength=V).astype(np.int64)
    d_masked = c.column_sums(raw, mask)
    assert np.array_equal(d_masked.to_host(), masked_sums.astype(np.uint32)) and 0 < masked_sums.sum() < all_sums.sum()
    with pytest.raises(E.CrgpuError) as ei:
        c.column_sums(raw, mask[: w.n_genes // 2])             # rows beyond the mask
    assert ei.value.code == EINVAL

    for sums, counts_arg, kw in ((all_sums, raw, dict()), (all_sums, raw, dict(recovered_cells=250)),
                                 (masked_sums, d_masked, dict()), (masked_sums, d_masked, dict(recovered_cells=250))):
        cols, ref = R.ordmag(sums, **kw)
        assert _bounds_are_safe(ref) and 0 < ref["filtered_bcs"] < V
        call = c.call_cells_ordmag(counts_arg, **kw)
        _check_call(call, cols, ref)
        # the filtered matrix == numpy's column selection of the raw one
        f_rank, f_indptr, f_indices, f_data = call.filtered_matrix(raw).download()
        e_indptr, e_indices, e_data = _csc_select(indptr, indices, data, cols)
        assert np.array_equal(f_rank, rank[cols])
        assert np.array_equal(f_indptr, e_indptr) and np.array_equal(f_indices, e_indices) and np.array_equal(f_data, e_data)
        # the called ranks close the seam to the probe entry points
        d_ranks = call.ranks_dev(raw)
        assert np.array_equal(d_ranks.to_host(), rank[cols])
        pb, pp, pc = counts.probe_triplets(n_probes)
        e_all, e_filt = np.zeros(n_probes, np.uint64), np.zeros(n_probes, np.uint64)
        np.add.at(e_all, pp, pc.astype(np.uint64))
        in_cells = np.isin(pb, rank[cols])
        np.add.at(e_filt, pp[in_cells], pc[in_cells].astype(np.uint64))
        all_, filt = counts.probe_metrics(n_probes, d_ranks)
        assert np.array_equal(all_, e_all) and np.array_equal(filt, e_filt) and 0 < filt.sum() < all_.sum()
    # a device column list is checked on the device
    bad = c.upload(np.array([0, V], np.uint64))
    mv = E.C.POINTER(E._lib.MatrixDevView)()
    assert c.L.crgpu_select_barcodes_cols_dev(c.h, raw._mv, E._p(bad), 2, E.C.byref(mv)) == EINVAL
    counts.free()
    c.close()
