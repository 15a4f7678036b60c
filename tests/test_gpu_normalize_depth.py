"""GPU tests of the depth normalisation (crgpu_normalize_depth_dev / Counts.normalize_depth, crgpu_select_features_dev /
Context.select_features_dev): the matrix, the read sums and the new read counts equal the numpy restatement
(tests/normalize_depth_numpy.py) run on Counts.molecules() of the same counts -- array equality on integers, no tolerance.  At
rate 1 the matrix must be the undrawn matrix the count stage itself assembled, which ties the run tally to the project's pinned
matrix without any random stream.

The records are the `small` and `long` sets of tests/test_gpu_subsample.py (its helpers are imported): 40 barcodes with about
3 000 molecules of 1 to 5 000 reads, one feature in both libraries of a barcode, a barcode of a single one-read molecule; and a
(barcode, feature) run of 600 molecules inside a barcode of 20 000.  They are the smallest shapes that reach every path of the
draw, a run across libraries and a run across many tiles and workgroup rounds of the compaction."""
import functools

import numpy as np
import pytest

import normalize_depth_numpy as N
import test_gpu_subsample as T

pytestmark = pytest.mark.gpu
EINVAL = -1
F = T.N_FEATURES
FCLASS = (np.arange(F) >= 30).astype(np.uint8)          # two classes
RATES = ([0.5, 0.0], [0.01, 0.5])
SUMS = ("raw_mapped_reads", "flt_mapped_reads", "reads_per_lib", "kept_reads_per_lib", "kept_molecules_per_lib")
_TABLE = {}                                             # kind -> (molecule table, raw matrix): the same in every context (asserted)


def _open(monkeypatch, kind, env=None, dense=None):
    """-> (context, counts, molecule table, raw matrix as a dict, (cell ranks, class masks))"""
    c = T._ctx(monkeypatch, env, dense)
    counts, m = T._counts(c, kind)
    mol = counts.molecules()
    mat = dict(rank=m.barcode_rank.copy(), indptr=m.indptr.copy(), indices=m.indices.copy(), data=m.data.copy())
    if kind in _TABLE:
        assert all(np.array_equal(mol[k], _TABLE[kind][0][k]) for k in mol)
        assert all(np.array_equal(mat[k], _TABLE[kind][1][k]) for k in mat)
    else:
        _TABLE[kind] = (mol, mat)
    return c, counts, mol, mat, T._cells(mol)


def _host(nd):
    """the device result as the dict the restatement returns (plus the column ranks)"""
    rank, indptr, indices, data = nd.matrix.download()
    out = dict(rank=rank, indptr=indptr, indices=indices, data=data, kept=nd.kept, result=nd.result)
    out.update({k: getattr(nd, k) for k in SUMS})
    nd.matrix.free()
    return out


@functools.lru_cache(maxsize=None)
def _reference(kind, frac, classes=True):
    """the restatement on the table of `kind`, computed once per rate list"""
    mol, mat = _TABLE[kind]
    ranks, ccm = T._cells(mol)
    if classes:
        return N.run(mol, list(frac), ranks, mat["rank"], F, FCLASS, 2, ccm)
    return N.run(mol, list(frac), ranks, mat["rank"], F)


def _assert_equal(got, want, what=""):
    for k in ("indptr", "indices", "data", "kept") + SUMS:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (what, k)


def _normalize(monkeypatch, kind, frac, env=None, dense=None, **kw):
    c, counts, mol, mat, (ranks, ccm) = _open(monkeypatch, kind, env, dense)
    args = dict(cell_ranks=ranks, feature_class=FCLASS, n_classes=2, cell_class_mask=ccm, want_kept=True)
    args.update(kw)
    got = _host(counts.normalize_depth(frac, **args))
    counts.free()
    c.close()
    return got, mol, mat, (ranks, ccm)


def _dense(indptr, indices, data, n_rows=F):
    out = np.zeros((len(indptr) - 1, n_rows), np.int64)
    out[np.repeat(np.arange(len(indptr) - 1), np.diff(indptr)), indices] = data
    return out


# ---- tests --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["small", "long"])
def test_all_rates_one_is_the_undrawn_matrix(monkeypatch, kind):
    got, mol, mat, _ = _normalize(monkeypatch, kind, [1.0, 1.0])
    for k in ("rank", "indptr", "indices", "data"):
        assert got[k].dtype == mat[k].dtype and np.array_equal(got[k], mat[k]), k
    assert np.array_equal(got["kept"], mol["read_count"])
    total = int(mol["read_count"].astype(np.int64).sum())
    assert got["raw_mapped_reads"].sum() == total and got["kept_reads_per_lib"].sum() == total
    assert np.array_equal(got["reads_per_lib"], got["kept_reads_per_lib"])
    assert np.array_equal(got["kept_molecules_per_lib"], np.bincount(mol["lib"], minlength=2))
    info = got["result"]
    planted = mol["read_count"]
    assert info["n_molecules"] == info["n_kept_molecules"] == len(planted) and info["n_triplets"] == len(mat["data"])
    assert (info["n_wave"], info["n_workgroup"]) == (int(((planted >= 64) & (planted < 4096)).sum()), int((planted >= 4096).sum()))
    assert info["n_lane"] + info["n_wave"] + info["n_workgroup"] == info["n_molecules"]
    if kind == "small":
        assert info["n_wave"] > 0 and info["n_workgroup"] > 0
        both = (mol["bc"] == np.unique(mol["bc"])[7]) & np.isin(mol["feature"], (3, 44))
        assert len(np.unique(mol["lib"][both])) == 2                   # a run across libraries
    else:
        sizes = np.bincount(np.searchsorted(np.unique(mol["bc"]), mol["bc"]))
        assert sizes.max() > 19_000 and got["data"].max() >= 600       # a run over many tiles inside a long barcode


def test_all_rates_zero(monkeypatch):
    got, mol, mat, _ = _normalize(monkeypatch, "small", [0.0, 0.0])
    assert np.array_equal(got["rank"], mat["rank"]) and np.array_equal(got["indptr"], np.zeros(len(mat["rank"]) + 1, np.int64))
    assert len(got["indices"]) == 0 and len(got["data"]) == 0 and not got["kept"].any()
    for k in ("raw_mapped_reads", "flt_mapped_reads", "kept_reads_per_lib", "kept_molecules_per_lib"):
        assert got[k].shape == (2,) and not got[k].any(), k
    assert np.array_equal(got["reads_per_lib"], np.bincount(mol["lib"], weights=mol["read_count"], minlength=2).astype(np.int64))
    assert got["result"]["n_triplets"] == 0 and got["result"]["n_kept_molecules"] == 0


@pytest.mark.parametrize("kind", ["small", "long"])
@pytest.mark.parametrize("frac", RATES, ids=["half_none", "hundredth_half"])
def test_equals_the_restatement(monkeypatch, kind, frac):
    got, mol, mat, (ranks, ccm) = _normalize(monkeypatch, kind, frac)
    want = _reference(kind, tuple(frac))
    _assert_equal(got, want)
    assert np.array_equal(got["rank"], mat["rank"])                    # the columns of the undrawn matrix, all of them
    assert got["result"]["n_triplets"] == len(want["data"]) and got["result"]["n_kept_molecules"] == int(np.count_nonzero(want["kept"]))
    # what the shapes are there for
    assert 0 < want["flt_mapped_reads"][0] < want["raw_mapped_reads"][0] and 0 < want["flt_mapped_reads"][1] < want["raw_mapped_reads"][1]
    assert 0 < len(want["data"]) < len(mat["data"]) and want["data"].max() > 1
    if kind == "small" and frac[0] == 0.01:
        emptied = (np.diff(want["indptr"]) == 0) & (np.diff(mat["indptr"]) > 0)
        assert emptied.any() and (np.diff(got["indptr"])[emptied] == 0).all()      # a barcode emptied by the draw keeps its column
    if frac[1] == 0.0:
        assert want["kept_molecules_per_lib"][1] == 0 and not got["kept"][mol["lib"] == 1].any()


@pytest.mark.parametrize("variant", ["lowered", "dense"])
def test_thresholds_and_dense_keys_change_nothing(monkeypatch, variant):
    kw = dict(env=T.LOWERED) if variant == "lowered" else dict(env=T.LOWERED, dense=True)
    frac = RATES[1]
    got, mol, _, _ = _normalize(monkeypatch, "small", frac, **kw)
    planted = mol["read_count"]
    info = got["result"]
    assert (info["n_wave"], info["n_workgroup"]) == (int(((planted >= 8) & (planted < 64)).sum()), int((planted >= 64).sum()))
    assert info["n_wave"] > 0 and info["n_workgroup"] >= 5
    _assert_equal(got, _reference("small", tuple(frac)), variant)
    if variant == "lowered":
        long_, _, _, _ = _normalize(monkeypatch, "long", RATES[0], env=T.LOWERED)
        _assert_equal(long_, _reference("long", tuple(RATES[0])), "long, lowered")


def test_agrees_with_subsampling_and_is_nested_in_the_rate(monkeypatch):
    c, counts, mol, mat, (ranks, ccm) = _open(monkeypatch, "small")
    frac = [0.01, 0.5]
    nd = _host(counts.normalize_depth(frac, cell_ranks=ranks, n_features=F, want_kept=True))
    ss = counts.subsample([frac], [T.R.PER_CELL], ranks, n_genomes=T.N_GENOMES, feature_genome=T.FEATURE_GENOME, seed=0)
    cols = np.searchsorted(mat["rank"], ranks)
    col_sums = np.add.reduceat(np.concatenate((nd["data"], [0])).astype(np.int64), nd["indptr"][:-1])
    col_sums[np.diff(nd["indptr"]) == 0] = 0
    assert np.array_equal(ss["umis_per_bc"][0].sum(0), col_sums[cols])
    assert ss["read_pairs"][0].sum() == nd["kept_reads_per_lib"].sum() == nd["raw_mapped_reads"].sum() == int(nd["kept"].sum())
    assert ss["umis"][0].sum() == nd["kept_molecules_per_lib"].sum() == nd["data"].sum()
    assert np.array_equal(nd["flt_mapped_reads"], [ss["read_pairs_per_bc"][0].sum()])         # one class, every cell of it
    # another seed is another draw; the same seed the same
    again = _host(counts.normalize_depth(frac, cell_ranks=c.upload(ranks), n_features=F, want_kept=True))       # a DeviceArray
    _assert_equal(again, nd, "second run")
    other = _host(counts.normalize_depth(frac, cell_ranks=ranks, n_features=F, want_kept=True, seed=1))
    assert not np.array_equal(other["kept"], nd["kept"])
    # nesting: the words do not depend on the rate
    quarter = _host(counts.normalize_depth([0.25, 0.25], n_features=F, want_kept=True))
    half = _host(counts.normalize_depth([0.5, 0.5], n_features=F, want_kept=True))
    assert (quarter["kept"] <= half["kept"]).all() and (quarter["kept"] < half["kept"]).any()
    assert (_dense(quarter["indptr"], quarter["indices"], quarter["data"]) <= _dense(half["indptr"], half["indices"], half["data"])).all()
    assert quarter["data"].sum() < half["data"].sum() and not quarter["flt_mapped_reads"].any()           # no cells given
    _assert_equal(quarter, N.run(mol, [0.25, 0.25], np.zeros(0, np.uint32), mat["rank"], F), "no cells, one class")
    counts.free()
    c.close()


def test_refusals_and_edges(monkeypatch):
    from cellranger_amd import engine as E

    c, counts, mol, mat, (ranks, ccm) = _open(monkeypatch, "small")
    kw = dict(cell_ranks=ranks, feature_class=FCLASS, n_classes=2, cell_class_mask=ccm)
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(E.CrgpuError) as e:
            counts.normalize_depth([0.5, bad], **kw)
        assert e.value.code == EINVAL, bad
    with pytest.raises(E.CrgpuError) as e:
        counts.normalize_depth([0.5, 0.5], **dict(kw, n_classes=1))                         # class 1 of 1
    assert e.value.code == EINVAL
    for n_classes in (0, 33):
        with pytest.raises(E.CrgpuError) as e:
            counts.normalize_depth([0.5, 0.5], n_features=F, n_classes=n_classes)
        assert e.value.code == EINVAL
    for bad_ranks in (ranks[::-1].copy(), np.array([5, 5], np.uint32)):
        with pytest.raises(E.CrgpuError) as e:
            counts.normalize_depth([0.5, 0.5], cell_ranks=bad_ranks, n_features=F)
        assert e.value.code == EINVAL
    with pytest.raises(E.CrgpuError):
        counts.normalize_depth([0.5], **kw)                                                 # one library, the counts have two
    with pytest.raises(E.CrgpuError):
        counts.normalize_depth([0.5, 0.5], n_features=F + 1)
    counts.free()
    # counts with no molecules: every column of the context's BarcodeIndex, empty; zero sums
    z = np.zeros(0, np.uint32)
    _, _, empty = c.count_host(F, z, z, np.zeros((0, T.UMI_LEN), np.uint8), z, np.zeros(0, np.uint8), want_dupinfo=False, want_counts=True)
    assert empty.n_molecules == 0
    got = _host(empty.normalize_depth([0.5, 0.5], want_kept=True, **kw))
    assert np.array_equal(got["rank"], mat["rank"]) and not got["indptr"].any() and len(got["indices"]) == 0 and len(got["kept"]) == 0
    assert all(got[k].shape == (2,) and not got[k].any() for k in SUMS)
    empty.free()
    c.close()


def test_select_features_and_the_filtered_matrix(monkeypatch):
    from cellranger_amd import engine as E

    c, counts, mol, mat, (ranks, ccm) = _open(monkeypatch, "long")
    nd = counts.normalize_depth([0.5, 0.5], n_features=F)
    m = nd.matrix
    rank, indptr, indices, data = m.download()
    rng = np.random.default_rng(3)
    mixed = (rng.integers(0, 3, F) > 0).astype(np.uint8)
    mixed[[0, 7, F - 1]] = 0, 0, 1                                       # the 600-molecule row leaves, the last row stays
    for name, mask in (("mixed", mixed), ("ones", np.ones(F, np.uint8)), ("zeros", np.zeros(F, np.uint8)), ("twos", 2 * mixed)):
        sub = c.select_features_dev(m, mask)
        got = sub.download()
        want = N.select_features(indptr, indices, data, mask)
        assert np.array_equal(got[0], rank), name                        # every column stays
        for g, w in zip(got[1:], want):
            assert g.dtype == w.dtype and np.array_equal(g, w), name
        sub.free()
        if name == "ones":
            assert np.array_equal(got[2], indices) and np.array_equal(got[3], data)
        if name == "mixed":
            assert 0 < len(got[2]) < len(indices) and got[2].max() == int(mixed.sum()) - 1
    assert indices.max() >= F - 10
    with pytest.raises(E.CrgpuError) as e:
        c.select_features_dev(m, np.ones(F - 10, np.uint8))              # a row of the matrix is past the mask
    assert e.value.code == EINVAL
    # the filtered matrix of main(): the cells' columns, then the targeted rows
    cols = np.searchsorted(rank, ranks).astype(np.uint64)
    by_cells = c.select_barcodes_dev(m, cols)
    filtered = c.select_features_dev(by_cells, mixed)
    got = filtered.download()
    want = N.select_features(*N.select_barcodes(indptr, indices, data, cols), mixed)
    assert np.array_equal(got[0], ranks)
    for g, w in zip(got[1:], want):
        assert np.array_equal(g, w)
    assert 0 < len(got[2]) < len(indices)
    for x in (filtered, by_cells, m):
        x.free()
    counts.free()
    c.close()
