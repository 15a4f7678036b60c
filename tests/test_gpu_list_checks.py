"""Every entry point that takes a list of columns or of barcode ranks, driven with the shapes at which the shared list checks of
csrc/stage_common.h (k_check_columns, k_check_ranks) can go wrong: length 0, 1 and 2, two equal neighbours, a descent, a last element
out of range, 257 entries whose only violation lies between entries 255 and 256 (the edge of the first workgroup of 256 threads), and
a valid list of 257 entries.

Column lists (a 300-column, 8-feature hand matrix of a 75 x 4 GelBeadAndProbe construct):
  matrix_summary, apply_minimum_umis, apply_mito_threshold, call_additional_cells   in range AND strictly ascending, else CRGPU_EINVAL
  rtl_gem_runs, rtl_medians, trim_molecule_barcodes                                 in range only: an unsorted list is taken as it is
Rank lists (a molecule table of a few hundred molecules): probe_metrics, probe_matrix, feature_metrics, subsample, normalize_depth
  strictly ascending, else CRGPU_EINVAL; a rank beyond the whitelist is no error (it has no molecule).
A list that is accepted gives what the stage's numpy restatement gives on that list; everything is compared for equality."""
import numpy as np
import pytest

import aggregates_numpy as AG
import emptydrops_numpy as ED
import matrix_summary_numpy as MS
import normalize_depth_numpy as ND
import subsample_numpy as SS
import targeted_metrics_numpy as TM

pytestmark = pytest.mark.gpu
EINVAL = -1
N_GEL, N_PROBE, V, F = 100, 4, 300, 8          # columns 0 .. 299 = canonical ranks 0 .. 299 of 400
N_RANKS, N_PROBES, UMI_LEN = 400, 16, 12
MITO = np.arange(F) < 2
_shared = {}


# ---- the lists --------------------------------------------------------------------------------------------------------------------
def _lists(bound, dtype):
    """bound: one past the largest valid element (the columns of the matrix, the ranks of the whitelist).
    -> (valid, unordered, beyond): dicts name -> list.  `unordered` lists are in range, `beyond` is ascending."""
    long = np.arange(257) + np.arange(257) // 7              # ascending with gaps, 0 .. 292
    assert long[-1] < bound and (np.diff(long) > 0).all()
    edge = long.copy()
    edge[256] = edge[255]                                    # the only violation: between entries 255 and 256
    assert (np.diff(edge) > 0).sum() == 255
    valid = {"none": [], "one": [6], "two": [6, 10], "long": long}
    unordered = {"equal": [6, 6], "descent": [10, 6], "edge": edge}
    beyond = {"beyond": [6, bound]}
    return tuple({k: np.asarray(v, dtype) for k, v in d.items()} for d in (valid, unordered, beyond))


def _refused(call, match=None):
    from cellranger_amd import engine as E

    with pytest.raises(E.CrgpuError, match=match) as e:
        call()
    assert e.value.code == EINVAL


# ---- the hand matrix ----------------------------------------------------------------------------------------------------------------
def _hand_matrix():
    """column k holds k % 4 entries (every fourth column is empty): features (3 k + 2 j) % 8, counts 1 .. 11"""
    indptr, indices, data = [0], [], []
    for k in range(V):
        fs = sorted((3 * k + 2 * j) % F for j in range(k % 4))
        indices += fs
        data += [1 + (7 * k + 5 * f) % 11 for f in fs]
        indptr.append(len(indices))
    return np.array(indptr, np.int64), np.array(indices, np.int32), np.array(data, np.int32)


def _device_matrix(c, indptr, indices, data):
    """MatrixDev whose column k is canonical rank k (as tests/test_gpu_emptydrops.py::_matrix builds it)"""
    n = len(indptr) - 1
    seen = np.zeros(c.n_canon, np.uint32)
    seen[:n] = 1
    c.set_counts(0, 0, seen)
    bc = np.repeat(np.arange(n, dtype=np.uint32), np.diff(indptr))
    m = c.assemble_matrix_dev(c.upload(bc), c.upload(indices.astype(np.uint32)), c.upload(data.astype(np.uint32)), len(bc))
    assert m.n_barcodes == n and m.nnz == len(bc)
    return m


def _well():
    if "well" not in _shared:
        import gpu_helpers as G

        c = G.fresh_ctx(dense=False)
        c.set_barcode_segments(0, [np.arange(N_GEL, dtype=np.uint32), np.arange(N_PROBE, dtype=np.uint32)], [16, 8])
        indptr, indices, data = _hand_matrix()
        m = _device_matrix(c, indptr, indices, data)
        tot = AG.column_sums(indptr, indices, data, np.ones(F, bool))
        mt = AG.column_sums(indptr, indices, data, MITO)
        d_tot, d_mt = c.column_sums(m), c.column_sums(m, MITO)
        assert np.array_equal(d_tot.to_host(), tot) and np.array_equal(d_mt.to_host(), mt) and (tot == 0).sum() == V // 4
        _shared["well"] = dict(c=c, m=m, indptr=indptr, indices=indices, data=data, tot=tot, mt=mt, d_tot=d_tot, d_mt=d_mt)
    return _shared["well"]


def _call(c, m, cols):
    from cellranger_amd import engine as E

    cols = np.ascontiguousarray(cols, dtype=np.uint64)
    return E.CellCall(c, c.upload(cols) if len(cols) else c.empty(0, np.uint64), len(cols), {"filtered_bcs": len(cols)}, m)


def _column_cases(strict):
    """(name, list, accepted) in a fixed order"""
    valid, unordered, beyond = _lists(V, np.uint64)
    cases = [(k, v, True) for k, v in valid.items()] + [(k, v, not strict) for k, v in unordered.items()]
    return cases + [(k, v, False) for k, v in beyond.items()]


# ---- column lists that must ascend -------------------------------------------------------------------------------------------------
def test_matrix_summary():
    from test_gpu_matrix_summary import _same

    w = _well()
    c, m = w["c"], w["m"]
    for name, cols, ok in _column_cases(strict=True):
        if not ok:
            _refused(lambda: c.matrix_summary(m, cols, n_features=F), "ascend" if name != "beyond" else "out of range")
            continue
        s = c.matrix_summary(m, cols, n_features=F, per_cell=True)
        ref = MS.summary(w["indptr"], w["indices"], w["data"], F, cols)
        _same(s, ref, dict(reads=None, cells=cols), per_cell=len(cols) > 0)
        assert s.classes[0]["cells_total_counts"] == int(w["tot"][cols.astype(np.int64)].sum()), name


def test_apply_minimum_umis():
    w = _well()
    c, m = w["c"], w["m"]
    for name, cols, ok in _column_cases(strict=True):
        if not ok:
            _refused(lambda: c.apply_minimum_umis(_call(c, m, cols), w["d_tot"], 8), "ascend" if name != "beyond" else "out of range")
            continue
        out = c.apply_minimum_umis(_call(c, m, cols), w["d_tot"], 8)
        exp = AG.apply_minimum_umis(cols, w["tot"], 8)
        assert out.n_cells == len(exp) and np.array_equal(out.cols_host(), exp), name
        assert name != "long" or 0 < len(exp) < len(cols)


def test_apply_mito_threshold():
    w = _well()
    c, m = w["c"], w["m"]
    for name, cols, ok in _column_cases(strict=True):
        if not ok:
            _refused(lambda: c.apply_mito_threshold(_call(c, m, cols), w["d_mt"], w["d_tot"], 30.0), "ascend" if name != "beyond" else "out of range")
            continue
        out, summary = c.apply_mito_threshold(_call(c, m, cols), w["d_mt"], w["d_tot"], 30.0)
        kept, removed, r_tot, r_pct = AG.apply_mito_threshold(cols, w["mt"], w["tot"], 30.0)
        assert out.n_cells == len(kept) and np.array_equal(out.cols_host(), kept), name
        assert np.array_equal(summary["cols"], removed) and np.array_equal(summary["total_umis"], r_tot.astype(np.uint32))
        assert summary["mt_pct"].tobytes() == r_pct.tobytes()
        assert name != "long" or (len(removed) > 0 and len(kept) > 0)


def test_call_additional_cells_on_the_hand_matrix():
    """eight features cannot give the ten distinct frequencies Simple Good-Turing asks for: an accepted list comes back as the call"""
    w = _well()
    c, m = w["c"], w["m"]
    for name, cols, ok in _column_cases(strict=True):
        if not ok:
            _refused(lambda: c.call_additional_cells(m, _call(c, m, cols), 100, 200, 5, num_sims=10), "ascending")
            continue
        ref = ED.find_nonambient(w["indptr"], w["indices"], w["data"], F, cols, 100, 200, 5, 10)
        a = c.call_additional_cells(m, _call(c, m, cols), 100, 200, 5, num_sims=10)
        assert a.status == ref["status"] == ED.STATUS_SGT, name
        assert a.metrics["n_ambient_used"] == ref["n_ambient_used"] and a.metrics["emptydrops_minimum_umis"] == ref["emptydrops_minimum_umis"]
        assert a.call.n_cells == len(cols) and np.array_equal(a.call.cols_host(), cols)


def test_call_additional_cells_marks_its_cells():
    """a 300-column, 60-feature planted well on which the step runs to its end: the cells are marked on the device, and no marked
    column may be a candidate"""
    import gpu_helpers as G
    from test_gpu_emptydrops import _check_integers

    indptr, indices, data, nf, kind = ED.make_well(1, n_features=60, n_cells=270, n_ambient=20, n_big_ambient=5, n_small_cells=5)
    assert len(kind) == V
    planted = np.flatnonzero(kind == 0)
    c = G.fresh_ctx()
    c.set_whitelist(0, np.arange(1024, dtype=np.uint32), length=16)
    m = _device_matrix(c, indptr, indices, data)
    for n in (1, 2, 257):
        cols = planted[:n].astype(np.uint64)
        ref = ED.find_nonambient(indptr, indices, data, nf, cols, 272, 300, 50, 10)
        assert ref["status"] == ED.STATUS_OK and len(ref["eval_cols"]) >= 270 - n
        a = c.call_additional_cells(m, _call(c, m, cols), 272, 300, 50, num_sims=10)
        _check_integers(a, ref)
        assert not np.isin(a.eval_cols, cols).any()
    for bad in (planted[[3, 3]], planted[[4, 3]], np.append(planted[:256], planted[255]), np.append(planted[:5], V)):
        _refused(lambda: c.call_additional_cells(m, _call(c, m, bad), 272, 300, 50, num_sims=10), "ascending")
    m.free()
    c.close()


# ---- column lists that need not ascend -----------------------------------------------------------------------------------------------
def _gem_runs_of(cols):
    """what k_rt_gem_runs reports of a cell list: a function of the SET of cells"""
    cells = np.unique(np.asarray(cols, np.int64))
    cpp = np.bincount(cells % N_PROBE, minlength=N_PROBE).astype(np.uint64)
    first = np.full(N_PROBE, 0xFFFFFFFFFFFFFFFF, np.uint64)
    for k in cells[::-1]:
        first[k % N_PROBE] = k
    per_gem = np.bincount(cells // N_PROBE, minlength=V // N_PROBE)
    return cpp, first, int((per_gem > 0).sum()), np.bincount(per_gem[per_gem > 0], minlength=N_PROBE + 1)


def test_rtl_gem_runs():
    w = _well()
    c, m = w["c"], w["m"]
    tags = c.rtl_tags(m, np.arange(N_PROBE, dtype=np.uint8), N_PROBE)
    for name, cols, ok in _column_cases(strict=False):
        if not ok:
            _refused(lambda: c.rtl_gem_runs(m, tags, _call(c, m, cols)), "out of range")
            continue
        runs = c.rtl_gem_runs(m, tags, _call(c, m, cols))
        cpp, first, gems, hist = _gem_runs_of(cols)
        assert runs.n_cells == len(cols) and runs.n_gems == V // N_PROBE, name
        assert np.array_equal(runs.cells_per_probe[:N_PROBE], cpp) and np.array_equal(runs.first_cell_col_per_probe[:N_PROBE], first), name
        assert np.array_equal(runs.cells_per_tag[:N_PROBE], cpp)                      # tag p = probe barcode p
        assert runs.gems_with_cells == gems and np.array_equal(runs.cells_per_gem_hist[:N_PROBE + 1], hist), name


def test_rtl_medians():
    """get_median_umi_per_cell over the list as it is given (an entry listed twice counts twice)"""
    w = _well()
    c, m, tot = w["c"], w["m"], w["tot"]
    for name, cols, ok in _column_cases(strict=False):
        if not ok:
            _refused(lambda: c.rtl_medians(w["d_tot"], _call(c, m, cols)), "out of range")
            continue
        nz, med = c.rtl_medians(w["d_tot"], _call(c, m, cols))
        for p in range(N_PROBE):
            vals = np.sort([int(tot[k]) for k in cols.astype(np.int64) if k % N_PROBE == p and tot[k] > 0])
            n = len(vals)
            want = 0 if not n else int(vals[n // 2]) if n % 2 else (int(vals[n // 2 - 1]) + int(vals[n // 2])) // 2
            assert (int(nz[p]), int(med[p])) == (n, want), (name, p)


def test_trim_molecule_barcodes():
    """the pass_filter list of MERGE_MOLECULES' barcode trimming: retained = the union with the barcodes of the molecules"""
    from cellranger_amd import engine as E

    c = _well()["c"]
    idx = np.sort((np.arange(500) * 37) % V).astype(np.uint64)      # the molecules' barcode_idx column, sorted by barcode
    for name, pf, ok in _column_cases(strict=False):
        d_idx = c.upload(idx)
        if not ok:
            with pytest.raises(E.CrgpuError) as e:
                c.trim_molecule_barcodes(d_idx, len(idx), V, pf, offset=7)
            assert e.value.code == EINVAL and "beyond" in str(e.value)
            continue
        keep = np.union1d(pf, idx)
        newpos = np.full(V, -1, np.int64)
        newpos[keep.astype(np.int64)] = np.arange(len(keep))
        retained, pf_new = c.trim_molecule_barcodes(d_idx, len(idx), V, pf, offset=7)
        assert np.array_equal(retained, keep.astype(np.uint64)), name
        assert np.array_equal(d_idx.to_host(), (7 + newpos[idx.astype(np.int64)]).astype(np.uint64))
        assert np.array_equal(pf_new, (7 + newpos[pf.astype(np.int64)]).astype(np.uint64))
    # the molecules' column goes through the same kernel: one index beyond the barcodes, at the edge of the first workgroup
    bad = idx[:257].copy()
    bad[256] = V
    with pytest.raises(E.CrgpuError) as e:
        c.trim_molecule_barcodes(c.upload(bad), len(bad), V)
    assert e.value.code == EINVAL


# ---- rank lists ---------------------------------------------------------------------------------------------------------------------
def _table():
    """450 molecules of 1 .. 4 reads on every second rank below 300, eight features, sixteen probes (two features share a probe, some
    molecules have none)"""
    if "table" not in _shared:
        import gpu_helpers as G
        from test_gpu_subsample import _umi

        mols = [(2 * b, (b + 3 * j) % F, 1 + (b + j) % 4, j + 1) for b in range(150) for j in range(1 + b % 5)]
        bc, feature, reads, k = (np.array(x, np.int64) for x in zip(*mols))
        rep = np.repeat(np.arange(len(bc)), reads)
        rep = rep[np.random.default_rng(3).permutation(len(rep))]
        umi = np.array([_umi(int(x)) for x in k], np.uint32)
        probe = np.where((feature + k) % 7 == 0, -1, feature // 2 + 4 * ((bc // 2) % 4)).astype(np.int32)      # -1: no probe
        n = len(rep)
        c = G.fresh_ctx()
        c.set_whitelist(0, np.arange(N_RANKS, dtype=np.uint32), length=16)      # rank == value
        r = dict(cb=bc[rep].astype(np.uint32), cb_qualn=np.full((n, 16), 70, np.uint8), flags=np.zeros(n, np.uint8))
        _, idx, _, _ = G.gpu_barcode_stage(c, r, n)                              # fills the tables the barcode index is made of
        assert np.array_equal(idx, r["cb"])
        c.set_key_layout(F, UMI_LEN, 1, 0)
        m, _, counts = c.count_host(F, idx, umi[rep], np.full((n, UMI_LEN), 70, np.uint8), feature[rep], r["flags"],
                                    probe_idx=probe[rep], want_dupinfo=False, want_counts=True)
        mol = counts.molecules()
        assert counts.n_molecules == len(bc) and np.array_equal(np.sort(mol["read_count"]), np.sort(reads))
        _shared["table"] = dict(c=c, counts=counts, mol=mol, probe=counts.probe_idx(), columns=m.barcode_rank.copy())
    return _shared["table"]


def _rank_cases():
    valid, unordered, beyond = _lists(N_RANKS, np.uint32)
    return [(k, v, True) for d in (valid, beyond) for k, v in d.items()] + [(k, v, False) for k, v in unordered.items()]


def _probe_triplets(t):
    """(barcode, probe, count) ascending over the molecules with a probe"""
    has = t["probe"] >= 0
    key = (t["mol"]["bc"][has].astype(np.uint64) << np.uint64(32)) | t["probe"][has].astype(np.uint64)
    uniq, cnt = np.unique(key, return_counts=True)
    return (uniq >> np.uint64(32)).astype(np.uint32), (uniq & np.uint64(0xFFFFFFFF)).astype(np.uint32), cnt.astype(np.uint32)


def test_probe_metrics():
    from test_gpu_probe_counts import _expected_metrics

    t = _table()
    trip = _probe_triplets(t)
    assert 100 < len(trip[0]) and trip[2].max() > 1
    for name, ranks, ok in _rank_cases():
        if not ok:
            _refused(lambda: t["counts"].probe_metrics(N_PROBES, ranks), "strictly ascending")
            continue
        all_, filt = t["counts"].probe_metrics(N_PROBES, ranks)
        e_all, e_filt = _expected_metrics(trip, N_PROBES, ranks)
        assert np.array_equal(all_, e_all) and np.array_equal(filt, e_filt), name
        assert name != "long" or 0 < filt.sum() < all_.sum()


def test_probe_matrix():
    from test_gpu_probe_counts import _expected_matrix

    t = _table()
    trip = _probe_triplets(t)
    for name, ranks, ok in _rank_cases():
        if not ok:
            _refused(lambda: t["counts"].probe_matrix(N_PROBES, ranks), "strictly ascending")
            continue
        pm = t["counts"].probe_matrix(N_PROBES, ranks)
        rank, indptr, indices, data = pm.download()
        e_indptr, e_indices, e_data = _expected_matrix(trip, ranks)
        assert np.array_equal(rank, ranks) and np.array_equal(indptr, e_indptr), name
        assert np.array_equal(indices, e_indices) and np.array_equal(data, e_data), name
        assert name != "long" or 0 < len(data) < len(trip[0])
        pm.free()


def test_feature_metrics():
    t = _table()
    for name, ranks, ok in _rank_cases():
        if not ok:
            _refused(lambda: t["counts"].feature_metrics(F, ranks), "strictly ascending")
            continue
        got = t["counts"].feature_metrics(F, ranks)
        exp = TM.tallies(t["mol"], F, [0], ranks)
        for k, e in zip(("num_umis", "num_reads", "num_umis_cells", "num_reads_cells"), exp):
            assert np.array_equal(got[k], e), (name, k)
        assert name != "long" or 0 < got["num_umis_cells"].sum() < got["num_umis"].sum()


def test_subsample():
    t = _table()
    types, rates = [SS.PER_CELL, SS.CELLS_ONLY], np.array([[0.5], [1.0]])
    mol = t["mol"]
    kept = SS.kept_all_tasks(mol["read_count"].astype(np.int64), mol["lib"].astype(np.int64), rates, 1, np.arange(len(mol["bc"])))
    for name, ranks, ok in _rank_cases():
        if not ok:
            _refused(lambda: t["counts"].subsample(rates, types, ranks, n_features=F), "strictly ascending")
            continue
        got = t["counts"].subsample(rates, types, ranks, n_features=F)
        want = SS.run(types, rates, mol, ranks, n_features=F, kept_reads=kept)
        for k in ("umis_per_bc", "read_pairs_per_bc", "features_det_per_bc", "read_pairs", "umis", "total_features_det", "any_reads"):
            assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (name, k)
        assert name != "long" or (0 < got["umis"][1, 0] < len(mol["bc"]) and got["umis_per_bc"][0].any())


def test_normalize_depth():
    t = _table()
    mol = t["mol"]
    kept = SS.kept(mol["read_count"].astype(np.int64), mol["lib"].astype(np.int64), np.array([0.5]), 0)
    for name, ranks, ok in _rank_cases():
        if not ok:
            _refused(lambda: t["counts"].normalize_depth([0.5], ranks, n_features=F), "strictly ascending")
            continue
        nd = t["counts"].normalize_depth([0.5], ranks, n_features=F, want_kept=True)
        want = ND.run(mol, [0.5], ranks, t["columns"], F, kept_reads=kept)
        rank, indptr, indices, data = nd.matrix.download()
        assert np.array_equal(rank, t["columns"]) and np.array_equal(indptr, want["indptr"]), name
        assert np.array_equal(indices, want["indices"]) and np.array_equal(data, want["data"]) and np.array_equal(nd.kept, want["kept"]), name
        for k in ("raw_mapped_reads", "flt_mapped_reads", "reads_per_lib", "kept_reads_per_lib", "kept_molecules_per_lib"):
            assert np.array_equal(getattr(nd, k), want[k]), (name, k)
        assert name != "long" or 0 < want["flt_mapped_reads"][0] < want["raw_mapped_reads"][0]
        nd.matrix.free()
