"""GPU parity tests of the multi-genome analysis (Context.multigenome / crgpu_multigenome_dev, Context.genome_totals,
Context.multigenome_from_matrix): GEM classes, the multiplet bootstrap and the count purities.

The expected values come from tests/multigenome_numpy.py, a numpy restatement of lib/python/cellranger/analysis/multigenome.py
:80-335 with the real np.random.seed(0) / np.random.choice.  EVERY comparison is equality: the calls, the per-sample class
counts, the per-sample thresholds as f64 bit patterns, the branch codes and every number of the result struct.  There is no
tolerance in this file.

Shapes: the three hand fixtures of a few cells (a branch that changes between samples, a pure species, an observed multiplet),
n = 0 / 1 / 2, the two ends of the draw's rejection mask (64, 65), the scan tile of the sum fallback (2048 cells) and its
successor, 5000 cells (several tiles, both LDS and device-memory rows) and one size just above the LDS limit with few samples."""
import os

import numpy as np
import pytest

import multigenome_numpy as R

pytestmark = pytest.mark.gpu
EINVAL, ERANGE = -1, -6
F1 = ([900, 800, 700, 650, 12, 3, 40, 0, 5], [10, 7, 0, 30, 600, 500, 40, 0, 450])
F2 = ([1200, 900, 2000, 1500, 0, 1100, 700, 1, 1300, 800, 950, 0], [0, 1, 2, 0, 1, 0, 0, 2, 1, 0, 0, 2])
F3 = ([500, 400, 450, 3], [2, 1, 350, 300])
LDS_LIMIT = 32768              # the default of CRGPU_MG_LDS_CELLS
# (Multiplets, genome0, genome1) of the unresampled seeded mixture, counted once with numpy: pins multigenome_numpy.mixture
MIX_OBSERVED = {"mix2048": (69, 1240, 739), "mix2049": (88, 1228, 733), "mix5000": (217, 3028, 1755)}

_REF = {}


def _inputs(name):
    """(c0, c1) of a named input: F1 .. F3, or 'mix<n>' / 'pure<n>' of the seeded mixture"""
    if name in ("F1", "F2", "F3"):
        c0, c1 = {"F1": F1, "F2": F2, "F3": F3}[name]
        return np.array(c0, np.int64), np.array(c1, np.int64)
    pure = name.startswith("pure")
    n = int(name[4:] if pure else name[3:])
    return R.mixture(n, n, pure)


def _reference(name, bootstraps):
    """the restatement's result, computed once per (input, samples) and shared; nobody writes into it"""
    key = (name, bootstraps)
    if key not in _REF:
        _REF[key] = R.run(*_inputs(name), bootstraps)
    return _REF[key]


def _bits(x):
    return np.asarray(x, np.float64).view(np.uint64)


def _same_f64(a, b):
    """bit for bit, None only with None"""
    if a is None or b is None:
        return a is None and b is None
    return np.array_equal(_bits(a), _bits(b))


def _check(got, ref):
    print("n %d observed %s thresholds %r branch %d | boot branches %s mean %.17g inferred %d lb %s ub %s" % (
        got.n, got.observed, got.obs_thresholds, got.obs_branch, np.bincount(got.boot_branch, minlength=4).tolist(),
        got.summary["mean"], got.summary["inferred_multiplets"], got.summary["rate_lb"], got.summary["rate_ub"]))
    assert got.n == ref["n"] == got.summary["observed_all"]
    assert got.call.dtype == np.uint8 and np.array_equal(got.call, ref["call"])
    assert np.array_equal(got.boot_counts, ref["boot_counts"])
    assert np.array_equal(_bits(got.boot_thresholds), _bits(ref["boot_thresholds"]))
    assert np.array_equal(got.boot_branch, ref["boot_branch"])
    assert _same_f64(got.obs_thresholds, ref["obs_thresh"]) and got.obs_branch == ref["obs_branch"]
    assert got.observed == ref["observed"] and got.summary["observed_multiplets"] == ref["observed"][0]
    assert got.purity_sums == ref["purity_sums"]
    assert np.array_equal(got.purity, ref["purity"], equal_nan=True)
    assert _same_f64(got.boot, ref["boot"])
    s = got.summary
    assert _same_f64(s["mean"], ref["mean"]) and s["inferred_multiplets"] == ref["inferred_multiplets"]
    assert _same_f64(s["rate"], ref["rate"]) and _same_f64(s["normalized_rate"], ref["normalized_rate"])
    assert _same_f64(s["rate_lb"], ref["rate_lb"]) and _same_f64(s["rate_ub"], ref["rate_ub"])


def _snapshot(g):
    """host copy of a result (outlives its context)"""
    return (g.call.copy(), g.boot_counts.copy(), _bits(g.boot_thresholds).copy(), g.boot_branch.copy(), _bits(g.boot).copy(),
            {k: v for k, v in g.res.items() if k != "generator_words"}, g.res["generator_words"])


def _same(a, b):
    for x, y in zip(a[:5], b[:5]):
        assert np.array_equal(x, y)
    assert a[5].keys() == b[5].keys()
    for k, v in a[5].items():
        assert np.array_equal(_bits(v), _bits(b[5][k])) if isinstance(v, float) else v == b[5][k], k


def _run(c, name, bootstraps):
    c0, c1 = _inputs(name)
    return c.multigenome(c0.astype(np.uint32), c1.astype(np.uint32), bootstraps)


# ---- the hand fixtures ------------------------------------------------------------------------------------------------------
def test_f1_a_branch_that_changes_between_samples():
    import gpu_helpers as G

    ref = _reference("F1", 1000)
    assert np.bincount(ref["boot_branch"], minlength=4).tolist() == [25, 975, 0, 0]      # the numpy side takes both branches
    assert int(((ref["boot_counts"][:, 1] == 0) | (ref["boot_counts"][:, 2] == 0)).sum()) == 21
    assert ref["call"].tolist() == [0, 0, 0, 0, 1, 1, 0, 0, 1]                           # the tie and the all-zero cell: genome0
    _check(_run(G.ctx(), "F1", 1000), ref)


def test_f2_pure_species_takes_the_sum_order():
    import gpu_helpers as G

    ref = _reference("F2", 1000)
    assert ref["obs_branch"] == 3 and np.bincount(ref["boot_branch"], minlength=4).tolist() == [29, 0, 0, 971]
    capped = sum(1 for (m, g0, g1), v in zip(ref["boot_counts"].tolist(), ref["boot"]) if g0 and g1 and v == m + g0 + g1 and v < m / (2 * (g0 / (g0 + g1)) * (g1 / (g0 + g1))))
    assert capped == 5
    _check(_run(G.ctx(), "F2", 1000), ref)


def test_f3_an_observed_multiplet():
    import gpu_helpers as G

    ref = _reference("F3", 1000)
    assert ref["observed"] == (1, 2, 1) and np.bincount(ref["boot_branch"], minlength=4).tolist() == [305, 695, 0, 0]
    assert int(((ref["boot_counts"][:, 1] == 0) | (ref["boot_counts"][:, 2] == 0)).sum()) == 355
    _check(_run(G.ctx(), "F3", 1000), ref)


# ---- tiny n -------------------------------------------------------------------------------------------------------------------
def test_tiny_n():
    import gpu_helpers as G

    c = G.ctx()
    for c0, c1 in (([7], [3]), ([0], [0]), ([40], [40])):                # n = 1: no generator output, every sample the same
        g = c.multigenome(np.array(c0, np.uint32), np.array(c1, np.uint32), 50)
        _check(g, R.run(c0, c1, 50))
        assert g.res["generator_words"] == 0 and (g.boot_counts == g.boot_counts[0]).all()
        assert g.boot_counts[0].tolist() == ([1, 0, 0] if c0[0] >= 10 and c1[0] >= 10 else [0, 1, 0])
    for c0, c1 in (([500, 3], [2, 300]), ([500, 300], [2, 3]), ([5, 5], [5, 5])):      # n = 2
        g = c.multigenome(np.array(c0, np.uint32), np.array(c1, np.uint32), 200)
        _check(g, R.run(c0, c1, 200))
        assert g.res["generator_words"] > 0
    g = c.multigenome(np.zeros(0, np.uint32), np.zeros(0, np.uint32), 1000)            # n = 0: zeroed, no error
    assert g.n == 0 and len(g.call) == 0 and not g.boot_counts.any() and not g.boot_thresholds.any()
    assert all(v == 0 for v in g.res.values())
    from cellranger_amd import engine as E
    assert E.multigenome_metrics(g, "GRCh38", "mm10") == {}


# ---- the draw's mask: n = 64 rejects nothing, n = 65 rejects the most ---------------------------------------------------------
@pytest.mark.parametrize("n", [64, 65])
def test_mask_edges(n):
    import gpu_helpers as G

    g = _run(G.ctx(), "mix%d" % n, 1000)
    _check(g, _reference("mix%d" % n, 1000))
    words = g.res["generator_words"]
    assert words % 3632 == 0 and words >= 1000 * n * (1 if n == 64 else 128 / 65)


# ---- scan tiles of the sum order, batches, LDS and device-memory rows ---------------------------------------------------------
@pytest.mark.parametrize("name", ["mix2048", "mix2049", "mix5000", "pure2048", "pure2049", "pure5000"])
def test_tiles_batches_and_row_placement(name, monkeypatch):
    """the same result with the default batch, with 1, 7 and 1000 samples per batch (fresh contexts: the switches are read when
    a context is created), with the rows in LDS and with the rows in device memory; pure*: most samples take the sum order"""
    import gpu_helpers as G

    B = 200
    ref = _reference(name, B)
    if name.startswith("pure"):
        taken = np.bincount(ref["boot_branch"], minlength=4)        # a sample without a c1 > c0 barcode takes the default
        assert ref["obs_branch"] == 3 and taken[3] > B // 2 and taken[1] == taken[2] == 0
    else:
        assert ref["obs_branch"] == 1 and (ref["boot_branch"] == 1).all() and ref["observed"] == MIX_OBSERVED[name]
    monkeypatch.delenv("CRGPU_MG_BATCH", raising=False)
    monkeypatch.delenv("CRGPU_MG_LDS_CELLS", raising=False)
    c = G.fresh_ctx()
    g = _run(c, name, B)
    _check(g, ref)
    first = _snapshot(g)
    c.close()
    settings = [("CRGPU_MG_BATCH", "1"), ("CRGPU_MG_BATCH", "7"), ("CRGPU_MG_BATCH", "1000"), ("CRGPU_MG_LDS_CELLS", "0")]
    if name.startswith("pure") and not name.endswith("5000"):
        settings = [("CRGPU_MG_BATCH", "7"), ("CRGPU_MG_LDS_CELLS", "0")]
    for key, value in settings:
        monkeypatch.delenv("CRGPU_MG_BATCH", raising=False)
        monkeypatch.delenv("CRGPU_MG_LDS_CELLS", raising=False)
        monkeypatch.setenv(key, value)
        cb = G.fresh_ctx()
        _same(first, _snapshot(_run(cb, name, B)))
        cb.close()


def test_batches_of_the_5000_cell_case_with_every_switch(monkeypatch):
    """n = 5000 with the device-memory rows AND small batches at once"""
    import gpu_helpers as G

    ref = _reference("mix5000", 200)
    monkeypatch.setenv("CRGPU_MG_BATCH", "7")
    monkeypatch.setenv("CRGPU_MG_LDS_CELLS", "0")
    c = G.fresh_ctx()
    _check(_run(c, "mix5000", 200), ref)
    c.close()


@pytest.mark.parametrize("name", ["mix%d" % (LDS_LIMIT + 3), "pure%d" % (LDS_LIMIT + 3), "mix%d" % LDS_LIMIT])
def test_just_above_and_at_the_lds_limit(name):
    import gpu_helpers as G

    _check(_run(G.ctx(), name, 20), _reference(name, 20))


# ---- the entry point ----------------------------------------------------------------------------------------------------------
def test_twice_on_one_context_one_sample_and_refusals():
    import gpu_helpers as G
    from cellranger_amd import engine as E

    c = G.ctx()
    a = _snapshot(_run(c, "mix2049", 200))
    _same(a, _snapshot(_run(c, "mix2049", 200)))
    assert a[6] > 0
    one = _run(c, "F3", 1)                                      # one sample: no bounds
    _check(one, _reference("F3", 1))
    assert one.res["rate_bounds_set"] == 0 and one.summary["rate_lb"] is None and one.summary["rate_ub"] is None
    assert _run(c, "F3", 2).res["rate_bounds_set"] == 1
    # the first samples of a longer call are the samples of a shorter one (one stream)
    assert np.array_equal(_run(c, "F1", 10).boot_counts, _reference("F1", 1000)["boot_counts"][:10])
    for bad in (0, E._lib.MG_MAX_BOOTSTRAPS + 1):
        with pytest.raises(E.CrgpuError) as ei:
            _run(c, "F3", bad)
        assert ei.value.code == EINVAL
    with pytest.raises(E.CrgpuError) as ei:                    # c0 + c1 beyond 32 bits
        c.multigenome(np.array([5, 0xFFFFFFF0], np.uint32), np.array([5, 0x20], np.uint32), 10)
    assert ei.value.code == ERANGE
    with pytest.raises(ValueError):
        c.multigenome(np.zeros(3, np.uint32), np.zeros(4, np.uint32))
    with pytest.raises(TypeError):                             # device counts of another width are not reinterpreted
        c.multigenome(c.upload(np.zeros(4, np.uint64)), c.upload(np.zeros(4, np.uint32)))
    # the metric names of the stage
    g = _run(c, "F3", 1000)
    m = E.multigenome_metrics(g, "GRCh38", "mm10")
    ref = _reference("F3", 1000)
    assert list(m) == ["filtered_bcs_observed_all", "filtered_bcs_observed_multiplets", "filtered_bcs_inferred_multiplets",
                       "filtered_bcs_inferred_multiplet_rate", "filtered_bcs_inferred_normalized_multiplet_rate",
                       "filtered_bcs_inferred_multiplet_rate_lb", "filtered_bcs_inferred_multiplet_rate_ub",
                       "GRCh38_filtered_bcs_mean_count_purity", "mm10_filtered_bcs_mean_count_purity",
                       "multi_filtered_bcs_mean_count_purity"]
    assert list(m.values()) == [4, 1, ref["inferred_multiplets"], ref["rate"], ref["normalized_rate"], ref["rate_lb"], ref["rate_ub"],
                                ref["purity"][0], ref["purity"][1], ref["purity"][2]]


# ---- per-genome totals --------------------------------------------------------------------------------------------------------
def _matrix(c, indptr, indices, data):
    """MatrixDev of a CSC whose column k is the k-th whitelist entry"""
    V = len(indptr) - 1
    seen = np.zeros(c.n_canon, np.uint32)
    seen[:V] = 1
    c.set_counts(0, 0, seen)
    bc = np.repeat(np.arange(V, dtype=np.uint32), np.diff(indptr))
    m = c.assemble_matrix_dev(c.upload(bc), c.upload(indices.astype(np.uint32)), c.upload(data.astype(np.uint32)), len(indices))
    assert m.n_barcodes == V and m.nnz == len(indices)
    return m


def test_genome_totals_and_the_top_two():
    import gpu_helpers as G
    from cellranger_amd import engine as E

    c = G.fresh_ctx()
    c.set_whitelist(0, np.arange(4096, dtype=np.uint32), length=16)
    rng = np.random.RandomState(4)
    V, NF = 700, 90
    dense = rng.poisson(0.4, (NF, V)) * rng.randint(1, 50, (NF, V))
    fg = (np.arange(NF) % 3).astype(np.uint8)
    fg[[5, 17, 40, 88]] = [3, 200, 255, 7]                    # not counted with three genomes
    indptr = np.concatenate([[0], np.cumsum((dense != 0).sum(axis=0))]).astype(np.int64)
    rows, cols = np.nonzero(dense.T)[1], np.nonzero(dense.T)[0]
    m = _matrix(c, indptr, rows, dense.T[cols, rows])
    expect = np.array([dense[fg == g].sum() for g in range(3)], np.uint64)
    got = c.genome_totals(m, fg, 3)
    assert got.dtype == np.uint64 and np.array_equal(got, expect) and expect.sum() < dense.sum()
    assert E.multigenome_top_two(got) == R.top_two(expect)
    assert np.array_equal(c.genome_totals(m, fg, 2), expect[:2])          # genome 2 is then uncounted as well
    assert np.array_equal(c.genome_totals(m, fg, 256)[:3], expect)
    with pytest.raises(E.CrgpuError) as ei:
        c.genome_totals(m, fg[:NF // 2], 3)                                # rows beyond feature_genome
    assert ei.value.code == EINVAL
    # a tie in the totals: the larger index first
    tie = np.zeros((3, 4), np.int64)
    tie[0] = [9, 0, 0, 1]
    tie[1] = [1, 2, 3, 4]
    tie[2] = [0, 5, 5, 0]
    tp = np.concatenate([[0], np.cumsum((tie != 0).sum(axis=0))]).astype(np.int64)
    tr, tc = np.nonzero(tie.T)[1], np.nonzero(tie.T)[0]
    mt = _matrix(c, tp, tr, tie.T[tc, tr])
    tot = c.genome_totals(mt, np.array([0, 1, 2], np.uint8), 3)
    assert tot.tolist() == [10, 10, 10] and E.multigenome_top_two(tot) == [1, 2] == R.top_two(tot)
    assert E.multigenome_top_two([10, 10, 3]) == [0, 1] and E.multigenome_top_two([3, 10, 3]) == [1, 2]
    c.close()


# ---- end to end ---------------------------------------------------------------------------------------------------------------
def test_end_to_end_from_reads_to_the_gem_classes(tmp_path):
    """a two-species well: reads -> pass A / B -> count stage -> raw MatrixDev -> OrdMag call -> filtered matrix ->
    multigenome_from_matrix (totals, top two, masked column sums, classes, bootstrap, purities) -> gem_classification.csv"""
    import gpu_helpers as G
    from cellranger_amd import engine as E
    from cellranger_amd import synth as S

    n_reads = 300_000
    w = S.Workload(n_total=n_reads, seed=S.SEED0 + 11, n_wl=50_000, n_cells=200, n_ambient=5000, n_genes=1000)
    r = w.host_reads(0, n_reads)
    # the species of a read follows a bit of its barcode, 3 % of the reads cross over; the genes of a species are one half
    rng = np.random.RandomState(8)
    half = w.n_genes // 2
    species = ((r["cb"] >> 7) & 1) ^ (rng.rand(n_reads) < 0.03)
    has = r["feature"] != 0xFFFFFFFF
    r["feature"][has] = (r["feature"][has] % half + species[has] * half).astype(np.uint32)
    fg = (np.arange(w.n_genes) >= half).astype(np.uint8)
    fg[np.arange(w.n_genes) % 50 == 49] = 2                   # a third, small genome
    fg[np.arange(w.n_genes) % 97 == 0] = 255                  # rows of no genome
    c = G.fresh_ctx()
    c.set_whitelist(0, w.wl_packed, length=16)
    _, _, _, dev = G.gpu_barcode_stage(c, r, n_reads)
    c.set_key_layout(w.n_genes, w.umi_len, 1, 0)
    d = [c.upload(r["umi"]), c.upload(r["umi_qualn"]), c.upload(r["feature"])]
    counts = c.count_records(c.records(n_reads, w.umi_len, dev["idx"], d[0], d[1], d[2], dev["flags"]))
    bcf, ftf, ctf = counts.triplets_dev()
    raw = c.assemble_matrix_dev(bcf, ftf, ctf, counts.n_triplets)
    call = c.call_cells_ordmag(raw, recovered_cells=200)
    filtered = call.filtered_matrix()
    assert 100 < filtered.n_barcodes < 1000
    g = c.multigenome_from_matrix(filtered, fg, 3, bootstraps=100)

    rank, indptr, indices, data = filtered.download()
    col_of = np.repeat(np.arange(filtered.n_barcodes), np.diff(indptr))
    totals = np.array([data[fg[indices] == k].sum() for k in range(3)], np.uint64)
    assert np.array_equal(g.totals, totals) and g.top_two == R.top_two(totals) == [0, 1]
    c0 = np.bincount(col_of, weights=data * (fg[indices] == 0), minlength=filtered.n_barcodes).astype(np.int64)
    c1 = np.bincount(col_of, weights=data * (fg[indices] == 1), minlength=filtered.n_barcodes).astype(np.int64)
    assert np.array_equal(g.count0.to_host(), c0.astype(np.uint32)) and np.array_equal(g.count1.to_host(), c1.astype(np.uint32))
    ref = R.run(c0, c1, 100)
    _check(g, ref)
    assert min(ref["observed"][1:]) > 20                      # both species are there

    _, canon_sorted = c.canon_order()
    barcodes = [bytes(row).decode() + "-1" for row in E.unpack_seqs(np.asarray(canon_sorted)[rank], 16)]
    path = tmp_path / "gem_classification.csv"
    E.write_gem_classification_csv(str(path), barcodes, g.count0.to_host(), g.count1.to_host(), g.call, "GRCh38", "mm10")
    names = ["GRCh38", "mm10", "Multiplet"]
    expect = "barcode,GRCh38,mm10,call" + os.linesep + "".join(
        "%s,%d,%d,%s%s" % (barcodes[k], c0[k], c1[k], names[ref["call"][k]], os.linesep) for k in range(len(barcodes)))
    with open(path, newline="") as f:
        text = f.read()
    assert text.split(os.linesep) == expect.split(os.linesep) and text == expect
    counts.free()
    c.close()
