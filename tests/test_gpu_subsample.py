"""GPU tests of the read subsampling (crgpu_subsample_dev / Counts.subsample): all seven outputs equal the numpy restatement
(tests/subsample_numpy.py) run on Counts.molecules() of the same counts -- array equality, every path of the draw (a molecule
per lane, per wave, per workgroup), every task type, across the two thresholds, the task batch and the grouping of tasks into
calls.

Inputs are small synthetic records: every (barcode, UMI) pair is distinct and the UMIs of a barcode differ in at least two
bases (a check digit), so that neither the UMI correction nor the low-support filter touches the planted read counts."""
import functools

import numpy as np
import pytest

import subsample_numpy as R

pytestmark = pytest.mark.gpu
EINVAL = -1
N_FEATURES, N_GENOMES, UMI_LEN = 50, 2, 12
FEATURE_GENOME = (np.arange(N_FEATURES) >= 30).astype(np.uint8)     # 30 features of genome 0, 20 of genome 1
TASK_TYPES = [R.PER_CELL, R.PER_CELL, R.CELLS_ONLY, R.BULK, R.PER_CELL]
RATES = np.array([[1.0, 1.0], [0.01, 0.01], [0.5, 0.0], [0.01, 0.5], [0.0, 0.0]])
LOWERED = {"CRGPU_SS_WAVE_MIN": "8", "CRGPU_SS_WG_MIN": "64"}
OUTPUTS = ("umis_per_bc", "read_pairs_per_bc", "features_det_per_bc", "read_pairs", "umis", "total_features_det", "any_reads")


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
def _umi(k):
    """UMI number k of a barcode: 11 base-4 digits of k and their sum mod 4 -- two UMIs differ in at least two bases"""
    digits = [(k >> (2 * i)) & 3 for i in range(11)]
    u = sum(digits) & 3
    for d in digits:
        u = (u << 2) | d
    return u


@functools.lru_cache(maxsize=None)
def _records(kind):
    """(whitelist, per-read arrays, planted) -- `small`: 40 barcodes, about 3 000 molecules, read counts 1, 3, 4, 5, 8 (Philox
    block edges), 70, 300 and 5 000; barcode 0 holds a single molecule of one read.  `long`: one barcode of about 20 000 molecules
    with a (barcode, feature) run of 600 (a cell of both genomes), beside four small ones."""
    rng = np.random.default_rng(11 if kind == "small" else 12)
    wl = np.unique(rng.integers(0, 1 << 32, 64, dtype=np.uint64).astype(np.uint32))
    mols = []  # (barcode position, feature, library, umi number, reads)
    if kind == "small":
        for b in range(40):
            n = 1 if b == 0 else int(rng.integers(20, 130))
            for k in range(n):
                mols.append([b, int(rng.integers(0, N_FEATURES)), int(rng.integers(0, 2)), k + 1, int(rng.choice([1, 1, 1, 2, 3, 4, 5, 8]))])
        mols[0][4] = 1
        for j, reads in zip((5, 40, 300, 700, 1500, 2000), (70, 300, 5000, 70, 300, 8)):
            mols[j][4] = reads
        for f in (3, 44):                       # one feature in both libraries of barcode 7
            mols += [[7, f, 0, 1000 + f, 2], [7, f, 1, 2000 + f, 3]]
    else:
        k = 0
        for b, n in ((2, 30), (9, 25), (17, 12), (30, 8), (41, 20_000)):
            for j in range(n):
                k += 1
                f = 7 if (b == 41 and j < 600) else int(rng.integers(0, N_FEATURES))
                mols.append([b, f, int(rng.integers(0, 2)), k, int(rng.choice([1, 1, 2, 3]))])
    m = np.array(mols, np.int64)
    rep = np.repeat(np.arange(len(m)), m[:, 4])
    rep = rep[rng.permutation(len(rep))]
    n = len(rep)
    r = dict(cb=wl[m[rep, 0]].astype(np.uint32), cb_qualn=np.full((n, 16), 70, np.uint8),
             umi=np.array([_umi(int(k)) for k in m[:, 3]], np.uint32)[rep], umi_qualn=np.full((n, UMI_LEN), 70, np.uint8),
             feature=m[rep, 1].astype(np.uint32), flags=m[rep, 2].astype(np.uint8))
    return wl, r, np.sort(m[:, 4])


def _counts(c, kind):
    """whitelist, barcode stage and count stage of the records: (Counts, raw Matrix)"""
    import gpu_helpers as G

    wl, r, _ = _records(kind)
    for lib in range(2):
        c.set_whitelist(lib, wl, length=16)
    _, idx, _, _ = G.gpu_barcode_stage(c, r, len(r["cb"]))
    assert (idx != 0xFFFFFFFF).all()
    c.set_key_layout(N_FEATURES, UMI_LEN, 2, 0)
    m, _, counts = c.count_host(N_FEATURES, idx, r["umi"], r["umi_qualn"], r["feature"], r["flags"], want_dupinfo=False, want_counts=True)
    return counts, m


def _cells(mol):
    """every second barcode of the table (the first one, with its single molecule, among them); cells of genome 0 only, of genome
    1 only, or of both, in turn"""
    ranks = np.unique(mol["bc"])[::2].astype(np.uint32)
    return ranks, np.array([(1, 2, 3)[i % 3] for i in range(len(ranks))], np.uint32)


def _ctx(monkeypatch, env=None, dense=None):
    import gpu_helpers as G

    for k in ("CRGPU_SS_WAVE_MIN", "CRGPU_SS_WG_MIN", "CRGPU_SS_TASK_BATCH"):
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)          # read when the context is created
    return G.fresh_ctx(dense=dense)


@functools.lru_cache(maxsize=None)
def _reference(kind, masked=False):
    """the restatement on the molecule table of `kind`, computed once (the table is the same in every context: asserted)"""
    mol, (ranks, cgm) = _REF_TABLE[kind], _cells(_REF_TABLE[kind])
    mask = _feature_mask() if masked else None
    return R.run(TASK_TYPES, RATES, mol, ranks, N_GENOMES, FEATURE_GENOME, cgm, feature_mask=mask, seed=1, n_features=N_FEATURES)


_REF_TABLE = {}


def _feature_mask():
    m = np.ones(N_FEATURES, np.uint8)
    m[[0, 7, 31, 44]] = 0
    return m


def _subsample(monkeypatch, kind, env=None, dense=None, **kw):
    """-> (device result, molecule table, raw matrix, cells) in a context of its own"""
    c = _ctx(monkeypatch, env, dense)
    counts, m = _counts(c, kind)
    mol = counts.molecules()
    if kind in _REF_TABLE:
        assert all(np.array_equal(mol[k], _REF_TABLE[kind][k]) for k in mol)
    else:
        _REF_TABLE[kind] = mol
    ranks, cgm = _cells(mol)
    args = dict(rates=RATES, task_types=TASK_TYPES, cell_ranks=ranks, n_genomes=N_GENOMES, feature_genome=FEATURE_GENOME,
                cell_genome_mask=cgm, seed=1)
    args.update(kw)
    got = counts.subsample(**args)
    mat = dict(rank=m.barcode_rank.copy(), indptr=m.indptr.copy(), indices=m.indices.copy(), data=m.data.copy())
    counts.free()
    c.close()
    return got, mol, mat, (ranks, cgm)


def _assert_equal(got, want, what=""):
    for k in OUTPUTS:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (what, k)


# ---- tests --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", [None, LOWERED], ids=["default", "lowered"])
def test_small_table_equals_the_restatement(monkeypatch, env):
    got, mol, mat, (ranks, cgm) = _subsample(monkeypatch, "small", env)
    planted = np.sort(mol["read_count"])
    assert len(mol["bc"]) > 2500 and len(np.unique(mol["bc"])) == 40 and len(np.unique(mol["lib"])) == 2
    for reads in (1, 3, 4, 5, 8, 70, 300, 5000):
        assert reads in planted                                    # the dedup left the planted read counts alone
    assert (np.bincount(np.searchsorted(np.unique(mol["bc"]), mol["bc"])) == 1).any()      # a barcode with a single molecule
    info = got["info"]
    assert info["n_molecules"] == len(mol["bc"]) and info["n_groups"] == 40 and info["n_active_tasks"] == 4
    if env is None:
        assert (info["n_wave"], info["n_workgroup"]) == (int(((planted >= 64) & (planted < 4096)).sum()), int((planted >= 4096).sum()))
    else:
        assert (info["n_wave"], info["n_workgroup"]) == (int(((planted >= 8) & (planted < 64)).sum()), int((planted >= 64).sum()))
        assert info["n_wave"] > 0 and info["n_workgroup"] >= 5
    assert info["n_lane"] + info["n_wave"] + info["n_workgroup"] == info["n_molecules"]
    want = _reference("small")
    _assert_equal(got, want)
    # what the shapes are there for
    assert not want["umis_per_bc"][4].any() and not got["read_pairs"][4].any()               # the all-zero rate row
    dead = (want["umis_per_bc"][1].sum(0) == 0) & (want["umis_per_bc"][0].sum(0) > 0)
    assert dead.any()                                                                        # a cell whose molecules all die at 0.01
    assert (cgm == 1).any() and (want["umis_per_bc"][0][1][cgm == 1] == 0).all()             # cells of genome 0 only
    assert want["umis"][2].sum() < want["umis"][0].sum() and (want["features_det_per_bc"][3] == 0).all()
    # rate 1.0, per cell: the raw matrix
    cols = np.searchsorted(mat["rank"], ranks)
    assert np.array_equal(mat["rank"][cols], ranks)
    for g in range(N_GENOMES):
        for ci, col in enumerate(cols):
            rows = mat["indices"][mat["indptr"][col]:mat["indptr"][col + 1]]
            data = mat["data"][mat["indptr"][col]:mat["indptr"][col + 1]]
            mine = FEATURE_GENOME[rows] == g
            is_cell = (cgm[ci] >> g) & 1
            assert got["umis_per_bc"][0, g, ci] == (data[mine].sum() if is_cell else 0)
            assert got["features_det_per_bc"][0, g, ci] == (mine.sum() if is_cell else 0)
    assert np.array_equal(got["read_pairs"][0], [mol["read_count"][FEATURE_GENOME[mol["feature"]] == g].sum() for g in range(2)])


@pytest.mark.parametrize("env", [None, LOWERED], ids=["default", "lowered"])
def test_long_group_and_long_run_cross_the_tiles(monkeypatch, env):
    got, mol, _, _ = _subsample(monkeypatch, "long", env)
    sizes = np.bincount(np.searchsorted(np.unique(mol["bc"]), mol["bc"]))
    assert sizes.max() > 19_000
    big = mol["bc"] == np.unique(mol["bc"])[np.argmax(sizes)]
    assert ((mol["feature"] == 7) & big).sum() >= 600                  # one (barcode, feature) run over many tiles of 64
    _assert_equal(got, _reference("long"))


def test_tasks_one_per_call_and_in_batches_of_two_give_the_same(monkeypatch):
    whole, _, _, _ = _subsample(monkeypatch, "small")
    _assert_equal(whole, _reference("small"))
    batched, _, _, _ = _subsample(monkeypatch, "small", {"CRGPU_SS_TASK_BATCH": "2"})
    assert batched["info"]["n_batches"] == 2 and whole["info"]["n_batches"] == 1
    _assert_equal(batched, whole, "batches of two")
    # one task per call, and the same call twice: one context
    c = _ctx(monkeypatch)
    counts, _ = _counts(c, "small")
    ranks, cgm = _cells(counts.molecules())
    kw = dict(cell_ranks=c.upload(ranks), n_genomes=N_GENOMES, feature_genome=FEATURE_GENOME, cell_genome_mask=cgm)   # a DeviceArray
    for t in range(len(TASK_TYPES)):
        one = counts.subsample(RATES[t:t + 1], TASK_TYPES[t:t + 1], **kw)
        for k in OUTPUTS[:-1]:
            assert np.array_equal(one[k][0], whole[k][t]), (t, k)
        assert np.array_equal(one["any_reads"], whole["any_reads"])
    again = [counts.subsample(RATES, TASK_TYPES, **kw) for _ in range(2)]
    _assert_equal(again[0], whole, "DeviceArray cells")
    _assert_equal(again[1], again[0], "second run")
    other = counts.subsample(RATES, TASK_TYPES, seed=2, **kw)
    assert not np.array_equal(other["umis"][1], whole["umis"][1]) and np.array_equal(other["umis"][0], whole["umis"][0])
    counts.free()
    c.close()


def test_feature_mask(monkeypatch):
    got, mol, _, _ = _subsample(monkeypatch, "small", LOWERED, feature_mask=_feature_mask())
    want = _reference("small", masked=True)
    _assert_equal(got, want)
    assert got["info"]["n_molecules"] == int(_feature_mask()[mol["feature"]].sum()) < len(mol["bc"])
    assert not got["total_features_det"][:, :, [0, 7, 31, 44]].any() and got["total_features_det"][0].any()


def test_dense_barcode_keys(monkeypatch):
    got, _, _, _ = _subsample(monkeypatch, "small", LOWERED, dense=True)
    _assert_equal(got, _reference("small"))


def test_nan_rates(monkeypatch):
    """a NaN for a library that has molecules: zeros; the same task list otherwise unchanged"""
    rates = RATES.copy()
    rates[1, 1] = np.nan
    got, _, _, _ = _subsample(monkeypatch, "small", rates=rates)
    want = _reference("small")
    for k in OUTPUTS[:-1]:
        assert not got[k][1].any(), k
        assert np.array_equal(np.delete(got[k], 1, 0), np.delete(want[k], 1, 0)), k
    assert got["info"]["n_active_tasks"] == 3


def test_edges_and_refusals(monkeypatch):
    from cellranger_amd import engine as E

    c = _ctx(monkeypatch)
    counts, _ = _counts(c, "small")
    mol = counts.molecules()
    ranks, cgm = _cells(mol)
    kw = dict(n_genomes=N_GENOMES, feature_genome=FEATURE_GENOME)
    # no cells: the per-cell arrays are empty, the totals stay
    got = counts.subsample(RATES, TASK_TYPES, np.zeros(0, np.uint32), **kw)
    want = R.run(TASK_TYPES, RATES, mol, np.zeros(0, np.uint32), N_GENOMES, FEATURE_GENOME, None, n_features=N_FEATURES)
    _assert_equal(got, want, "no cells")
    assert got["umis_per_bc"].shape == (5, 2, 0) and got["umis"][0].sum() == len(mol["bc"]) and not got["umis"][2].any()
    for bad_ranks in (ranks[::-1].copy(), np.array([5, 5], np.uint32)):
        with pytest.raises(E.CrgpuError) as e:
            counts.subsample(RATES, TASK_TYPES, bad_ranks, **kw)
        assert e.value.code == EINVAL
    for bad in (1.5, -0.25):
        rates = RATES.copy()
        rates[2, 0] = bad
        with pytest.raises(E.CrgpuError) as e:
            counts.subsample(rates, TASK_TYPES, ranks, **kw)
        assert e.value.code == EINVAL
    for kwargs in (dict(n_genomes=9, n_features=N_FEATURES), dict(n_genomes=1, feature_genome=FEATURE_GENOME)):       # genome 1 of 1
        with pytest.raises(E.CrgpuError) as e:
            counts.subsample(RATES, TASK_TYPES, ranks, **kwargs)
        assert e.value.code == EINVAL
    with pytest.raises(E.CrgpuError):
        counts.subsample(RATES[:, :1], TASK_TYPES, ranks, **kw)                                # one library, the counts have two
    with pytest.raises(E.CrgpuError):
        counts.subsample(RATES, [0, 1, 2, 3, 0], ranks, **kw)                                  # an unknown task type
    counts.free()
    # counts with no molecules
    z = np.zeros(0, np.uint32)
    _, _, empty = c.count_host(N_FEATURES, z, z, np.zeros((0, UMI_LEN), np.uint8), z, np.zeros(0, np.uint8), want_dupinfo=False, want_counts=True)
    assert empty.n_molecules == 0
    got = empty.subsample(RATES, TASK_TYPES, ranks, cell_genome_mask=cgm, **kw)
    for k in OUTPUTS:
        assert not got[k].any(), k
    assert got["umis_per_bc"].shape == (5, 2, len(ranks)) and got["any_reads"].shape == (2, 2)
    empty.free()
    c.close()
