"""GPU tests of the targeted-metrics entry points: the per-feature tallies of the molecule table (crgpu_feature_metrics_dev), the
enrichment call (crgpu_rpu_gmm_dev) and the stage's summary (engine.targeted_metrics).

Tallies: the expected values are the restatement tests/targeted_metrics_numpy.py (np.add.at, the reference's chunk function) over
Counts.molecules() of the same counts; everything is compared for equality.  The 64-bit accumulation past 2^32 cannot be reached
at these sizes through the public interface (a feature would need more than 4 G reads): it is not faked here; the carry of the
u32 LDS counters is the arithmetic of the matrix summary's, and k_fm_slab_sum adds in 64 bits.

Fit: the golden file tests/golden/targeted_metrics_reference.npz holds the outputs of the reference's own fit_enrichments for the
fixtures (n = 130, 320 and 600 genes; one per guard), the restatement's per-start likelihoods and iteration counts, and the
conditions checked while recording (the gap between the two best starts, every posterior's distance from 0.5, every start's
distance from the stopping bound), so that equality is a fair demand: the threshold, the class counts, the per-gene flags, the
winner and every start's iteration count are compared for equality, no start and no gene left out.  The floats are held within
`fit_bound` of the golden file: 16 times the largest relative movement of the restatement's own parameters and likelihoods over 8
seeded permutations of each fixture's genes (gene order is arbitrary to the reference; reordering changes nothing but the order of
its sums, which is the freedom the device takes).  Measured 1.6e-14, bound 2.6e-13 (DESIGN.md "Targeted metrics")."""
import functools
import math
import os

import numpy as np
import pytest

import targeted_metrics_numpy as R

pytestmark = pytest.mark.gpu
EINVAL = -1
N_1M = 1_000_000
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "targeted_metrics_reference.npz")
SLICE_MAX = (160 * 1024 - 64) // 16      # FM_SLICE_MAX: features per LDS slice by default
TALLY_KEYS = ("num_umis", "num_reads", "num_umis_cells", "num_reads_cells")


@functools.lru_cache(maxsize=None)
def golden():
    return dict(np.load(GOLDEN))


# ---- tallies --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _reads(kind):
    """one_lib / two_libs: the 1 M-read, 300-cell input of tests/test_gpu_probe_counts.py.  hot: 2^17 reads over 2 000 barcodes, 40 %
    of them on one feature, the rest on features 0, slice - 1, slice, n_features - 1 and 300 random ones"""
    from cellranger_amd import synth as S

    if kind != "hot":
        n_libs = 2 if kind == "two_libs" else 1
        w = S.Workload(n_total=N_1M, seed=S.SEED0 + 3, n_cells=300, n_ambient=20000, n_libs=n_libs)
        return w, n_libs, w.host_reads(0, N_1M), N_1M
    n = 1 << 17
    w = S.Workload(n_total=n, seed=S.SEED0 + 11, n_cells=300, n_ambient=20000)
    r = w.host_reads(0, n)
    rng = np.random.default_rng(17)
    canon_sorted = np.sort(w.wl_packed)
    ranks = np.sort(rng.choice(len(canon_sorted), 2000, replace=False))
    ranks[0], ranks[-1] = 0, len(canon_sorted) - 1      # the first and the last barcode rank
    r["cb"][:] = canon_sorted[ranks[rng.integers(0, 2000, n)]]
    r["cb_qualn"][:] &= 0x7F
    r["flags"][:] &= 0xEF      # FLAG_CB_HAS_N
    r["umi"][:] = rng.integers(0, 1 << 14, n).astype(np.uint32)      # few UMIs: molecules of several reads
    r["umi_qualn"][:] &= 0x7F
    pool = np.concatenate([[0, SLICE_MAX - 1, SLICE_MAX, w.n_genes - 1], rng.choice(w.n_genes, 300, replace=False)]).astype(np.uint32)
    f = pool[rng.integers(0, len(pool), n)]
    f[rng.random(n) < 0.4] = 12345
    r["feature"][:] = f
    return w, 1, r, n


def _count(monkeypatch, kind, lds, dense=None):
    import gpu_helpers as G

    if lds is None:
        monkeypatch.delenv("CRGPU_FM_LDS_FEATURES", raising=False)
    else:
        monkeypatch.setenv("CRGPU_FM_LDS_FEATURES", str(lds))      # read when the context is created
    w, n_libs, r, n = _reads(kind)
    c = G.fresh_ctx(dense=dense)
    for lib in range(n_libs):
        c.set_whitelist(lib, w.wl_packed, length=16)
    _, _, _, dev = G.gpu_barcode_stage(c, r, n)
    c.set_key_layout(w.n_genes, w.umi_len, n_libs, 0)
    d = [c.upload(r["umi"]), c.upload(r["umi_qualn"]), c.upload(r["feature"])]
    counts = c.count_records(c.records(n, w.umi_len, dev["idx"], d[0], d[1], d[2], dev["flags"]))
    c.synchronize()
    return c, counts, w, n_libs, (dev, d)


def _cell_sets(mol):
    with_mol = np.unique(mol["bc"]).astype(np.uint32)
    return {"none": np.zeros(0, np.uint32), "third": with_mol[::3].copy(), "all": with_mol}


def _check_tallies(counts, mol, n_features, libs, cells):
    got = counts.feature_metrics(n_features, cells, libs=libs)
    exp = R.tallies(mol, n_features, libs, cells)
    for k, e in zip(TALLY_KEYS, exp):
        assert got[k].dtype == np.uint64 and np.array_equal(got[k], e), (k, libs, len(cells))
    return got


@pytest.mark.parametrize("lds", [None, 0, 1, 7])
@pytest.mark.parametrize("kind", ["one_lib", "two_libs"])
def test_tallies_equal_the_restatement(kind, lds, monkeypatch):
    """the 1 M-read well, one library and two: no cells, every third barcode with molecules, all of them; every lib_mask; the LDS
    slices by default (4 of them), one feature per slice, seven, and the counters in device memory"""
    c, counts, w, n_libs, keep = _count(monkeypatch, kind, lds)
    mol = counts.molecules()
    assert counts.n_molecules > 300_000 and len(np.unique(mol["feature"])) > 5_000      # not vacuous
    sets = _cell_sets(mol)
    masks = [[0]] if n_libs == 1 else [[0], [1], [0, 1]]
    for libs in masks:
        got = _check_tallies(counts, mol, w.n_genes, libs, sets["third"])
        assert 0 < got["num_umis_cells"].sum() < got["num_umis"].sum() < got["num_reads"].sum()
    for name in ("none", "all"):
        got = _check_tallies(counts, mol, w.n_genes, masks[-1], sets[name])
        assert np.array_equal(got["num_umis_cells"], got["num_umis"] if name == "all" else np.zeros(w.n_genes, np.uint64))
    if n_libs == 2:      # a scalar library index is a mask of one
        assert np.array_equal(counts.feature_metrics(w.n_genes, sets["third"], libs=1)["num_reads"], R.tallies(mol, w.n_genes, [1], sets["third"])[1])
    counts.free()
    c.close()


def test_tallies_under_dense_barcode_keys(monkeypatch):
    c, counts, w, n_libs, keep = _count(monkeypatch, "one_lib", None, dense=True)
    mol = counts.molecules()
    for cells in _cell_sets(mol).values():
        _check_tallies(counts, mol, w.n_genes, [0], cells)
    # a DeviceArray of ranks is taken as it is; None means no cells
    third = _cell_sets(mol)["third"]
    a, b = counts.feature_metrics(w.n_genes, c.upload(third)), counts.feature_metrics(w.n_genes, None)
    assert np.array_equal(a["num_reads_cells"], R.tallies(mol, w.n_genes, [0], third)[3]) and not b["num_umis_cells"].any()
    counts.free()
    c.close()


@pytest.mark.parametrize("lds", [None, 0, 1, 7])
def test_tallies_of_a_hot_feature_that_straddles_the_slices(lds, monkeypatch):
    c, counts, w, n_libs, keep = _count(monkeypatch, "hot", lds)
    mol = counts.molecules()
    share = np.bincount(mol["feature"], minlength=w.n_genes)
    assert share[12345] > 0.3 * counts.n_molecules and mol["read_count"].max() > 1
    assert all(share[f] > 0 for f in (0, SLICE_MAX - 1, SLICE_MAX, w.n_genes - 1))
    assert mol["bc"].min() == 0 and mol["bc"].max() == len(w.wl_packed) - 1
    for cells in _cell_sets(mol).values():
        _check_tallies(counts, mol, w.n_genes, [0], cells)
    counts.free()
    c.close()


def test_tallies_error_returns(monkeypatch):
    from cellranger_amd import engine as E

    c, counts, w, n_libs, keep = _count(monkeypatch, "hot", None)
    mol = counts.molecules()
    cells = _cell_sets(mol)["third"]
    L, h = c.L, c.h
    out = np.zeros(w.n_genes, np.uint64)
    from cellranger_amd._lib import ptr
    d_cells = c.upload(cells)
    args = (E._p(d_cells), len(cells), ptr(out), None, None, None)
    assert L.crgpu_feature_metrics_dev(h, counts.h, w.n_genes, 0, *args) == EINVAL and b"empty library mask" in L.crgpu_last_error(h)
    assert L.crgpu_feature_metrics_dev(h, counts.h, w.n_genes, 2, *args) == EINVAL and b"outside the key layout" in L.crgpu_last_error(h)
    assert L.crgpu_feature_metrics_dev(h, counts.h, w.n_genes - 1, 1, *args) == EINVAL and b"n_features" in L.crgpu_last_error(h)
    assert L.crgpu_feature_metrics_dev(h, counts.h, w.n_genes, 1, None, 3, ptr(out), None, None, None) == EINVAL
    for bad in (cells[::-1].copy(), np.repeat(cells[:4], 2)):
        with pytest.raises(E.CrgpuError, match="strictly ascending"):
            counts.feature_metrics(w.n_genes, bad)
    # every output may be NULL; n_cells == 0 is no error
    assert L.crgpu_feature_metrics_dev(h, counts.h, w.n_genes, 1, None, 0, None, None, None, None) == 0
    assert L.crgpu_feature_metrics_dev(h, counts.h, w.n_genes, 1, *args) == 0 and np.array_equal(out, R.tallies(mol, w.n_genes, [0], cells)[0])
    counts.free()
    c.close()


# ---- the fit ----------------------------------------------------------------------------------------------------------------------
def _rel(a, b):
    return abs(a - b) / abs(b)


def _same_or_nan(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == b


@pytest.fixture(scope="module")
def fit_ctx():
    import gpu_helpers as G

    c = G.fresh_ctx()
    yield c
    c.close()


_FITS = {}


def _run_fit(c, name):
    """one device fit per fixture, shared by the tests below and left unchanged"""
    if name not in _FITS:
        g = golden()
        _FITS[name] = c.rpu_gmm(g[name + "_values"], g[name + "_labels"], want_starts=True)
    return _FITS[name]


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_fit_equals_the_reference(name, fit_ctx):
    g = golden()
    bound = float(g["fit_bound"])
    assert 0 < float(g["fit_movement"]) * 16 == bound < 1e-11
    gap, post_margin, stop_margin = g[name + "_conditions"]
    assert gap >= 1e-8 and post_margin >= 1e-6 and stop_margin >= 1e-9      # the conditions under which equality is a fair demand
    res = _run_fit(fit_ctx, name)
    p, cs = g[name + "_ref_params"], g[name + "_ref_class"]
    print(name, "device", [res[k] for k in R.FIT_KEYS], "reference", list(p), "rel", [_rel(res[k], v) for k, v in zip(R.FIT_KEYS, p)])
    assert res["fitted"] == 1 and res["n_starts"] == R.N_STARTS and res["in_lds"] == 1
    assert res["log_rpu_threshold"] == p[0]
    assert [res[k] for k in R.CLASS_KEYS] == list(cs)
    assert np.array_equal(res["enriched"], g[name + "_enriched"])
    assert res["winner"] == int(g[name + "_winner"])
    for k, v in zip(R.FIT_KEYS[1:], p[1:]):
        assert _rel(res[k], v) <= bound, (k, res[k], v)
    assert res["sd_high"] == res["sd_low"] > 50      # the quirk: the tied PRECISION, twice
    assert _rel(res["max_lk"], float(g[name + "_restate_max_lk"])) <= bound
    # per start: no start left out
    lks, its = g[name + "_restate_lks"], g[name + "_restate_its"]
    assert len(lks) == R.N_STARTS == len(res["start_lk"])
    worst = np.max(np.abs(res["start_lk"] - lks) / np.abs(lks))
    print(name, "largest relative difference of a start's likelihood", worst, "iterations differ at", np.flatnonzero(res["start_iters"] != its))
    assert np.array_equal(res["start_iters"], its)
    assert worst <= bound
    assert res["max_lk"] == res["start_lk"][res["winner"]] == res["start_lk"].max()


@pytest.mark.parametrize("name", ["a", "c"])
def test_fit_is_reproducible_and_blind_to_the_gene_order(name, fit_ctx):
    g = golden()
    first = _run_fit(fit_ctx, name)
    again = fit_ctx.rpu_gmm(g[name + "_values"], g[name + "_labels"], want_starts=True)
    for k in R.FIT_KEYS + R.CLASS_KEYS + ("max_lk", "winner"):
        assert np.float64(first[k]).tobytes() == np.float64(again[k]).tobytes(), k
    assert first["start_lk"].tobytes() == again["start_lk"].tobytes() and first["start_iters"].tobytes() == again["start_iters"].tobytes()
    rev = fit_ctx.rpu_gmm(g[name + "_values"][::-1].copy(), g[name + "_labels"][::-1].copy())
    assert rev["log_rpu_threshold"] == first["log_rpu_threshold"] and rev["winner"] == first["winner"]
    assert [rev[k] for k in R.CLASS_KEYS] == [first[k] for k in R.CLASS_KEYS]
    assert np.array_equal(rev["enriched"][::-1], first["enriched"])


def test_fit_from_device_memory_equals_the_fit_from_lds(fit_ctx, monkeypatch):
    """CRGPU_GMM_LDS_VALUES=0: the values are read from device memory; the arithmetic and its order are the same"""
    import gpu_helpers as G

    g = golden()
    first = _run_fit(fit_ctx, "b")
    monkeypatch.setenv("CRGPU_GMM_LDS_VALUES", "0")
    c = G.fresh_ctx()
    res = c.rpu_gmm(g["b_values"], g["b_labels"], want_starts=True)
    assert res["in_lds"] == 0 and first["in_lds"] == 1
    assert res["start_lk"].tobytes() == first["start_lk"].tobytes() and np.array_equal(res["start_iters"], first["start_iters"])
    for k in R.FIT_KEYS + R.CLASS_KEYS:
        assert np.float64(res[k]).tobytes() == np.float64(first[k]).tobytes(), k
    c.close()


@pytest.mark.parametrize("guard", ["empty", "no_offtarget", "too_few", "no_targeted"])
def test_guards_return_the_reference_pattern_without_a_fit(guard, fit_ctx):
    g = golden()
    vals, lab = g["guard_%s_values" % guard], g["guard_%s_labels" % guard]
    res = fit_ctx.rpu_gmm(vals, lab, want_starts=True)
    assert res["fitted"] == 0 and res["n_starts"] == 0 and res["winner"] == 0xFFFFFFFF      # nothing was launched
    assert np.isnan(res["start_lk"]).all() and not res["start_iters"].any()
    for k, v in zip(R.FIT_KEYS, g["guard_%s_ref_params" % guard]):
        assert _same_or_nan(res[k], float(v)), (k, res[k], v)
    for k, v in zip(R.CLASS_KEYS, g["guard_%s_ref_class" % guard]):
        assert _same_or_nan(res[k], float(v)), (k, res[k], v)
    if guard == "no_offtarget":
        assert np.array_equal(res["enriched"], (vals >= 0).astype(np.uint8)) and res["log_rpu_threshold"] == 0.0


def test_fit_refuses_values_that_are_not_finite(fit_ctx):
    from cellranger_amd import engine as E

    g = golden()
    v = g["a_values"].copy()
    v[7] = np.nan
    with pytest.raises(E.CrgpuError, match="not finite"):
        fit_ctx.rpu_gmm(v, g["a_labels"])


# ---- the stage's summary --------------------------------------------------------------------------------------------------------------
def _same_summary(got, ref, bound, tallies, is_targeted, is_gex):
    """the fit's floats within `bound` (relative), the means and cvs within R.float_bounds (derived there), everything else equal"""
    assert sorted(got) == sorted(ref)
    fb = R.float_bounds(R.feature_summary_df(*[tallies[k] for k in TALLY_KEYS], is_targeted, is_gex))
    for k, v in ref.items():
        a, v = float(got[k]), float(v)
        if math.isnan(a) and math.isnan(v):
            continue
        if k.startswith("lrpu_fitted_"):
            assert _rel(a, v) <= bound, (k, a, v)
        elif k in fb:
            assert abs(a - v) <= (fb[k][0] * abs(v) + fb[k][1]) * 2.0 ** -52, (k, a, v)
        else:
            assert a == v, (k, a, v)


def test_targeted_metrics_equal_the_golden_dict(fit_ctx):
    """end to end on the recorded small well: tallies -> statistics -> fit -> the summary dict and the enriched_rpu column"""
    from cellranger_amd import engine as E

    g = golden()
    t = {k: g["e2e_" + k] for k in TALLY_KEYS}
    med_u, med_g, num_cells, total_reads, frac_on, frac_off = g["e2e_args"]
    s, col = E.targeted_metrics(fit_ctx, t, g["e2e_is_targeted"], (med_u, med_g), int(num_cells), int(total_reads), float(frac_on), float(frac_off),
                                is_gex=g["e2e_is_gex"])
    ref = dict(zip([str(k) for k in g["e2e_keys"]], g["e2e_values"]))
    _same_summary(s, ref, float(g["fit_bound"]), t, g["e2e_is_targeted"], g["e2e_is_gex"])
    assert np.array_equal(col, g["e2e_enriched_rpu"], equal_nan=True) and 0 < np.nansum(col) < len(col)
    # the disable_rpu_enrichments rule: with a third of the reads the on-target mean falls below 2.5 and too few targets stay enriched
    low = dict(t)
    low["num_reads"], low["num_reads_cells"] = np.maximum(t["num_reads"] // 3, t["num_umis"]), np.maximum(t["num_reads_cells"] // 3, t["num_umis_cells"])
    s2, col2 = E.targeted_metrics(fit_ctx, low, g["e2e_is_targeted"], (med_u, med_g), int(num_cells), int(total_reads), float(frac_on), float(frac_off),
                                  is_gex=g["e2e_is_gex"])
    st = E.targeted_rpu_stats(low["num_umis"], low["num_reads"], low["num_umis_cells"], low["num_reads_cells"], g["e2e_is_targeted"], g["e2e_is_gex"])
    fe = fit_ctx.rpu_gmm(st["q_value"], st["q_label"])
    ref2, refcol2 = R.targeted_metrics(low["num_umis"], low["num_reads"], low["num_umis_cells"], low["num_reads_cells"], g["e2e_is_targeted"], g["e2e_is_gex"],
                                       med_u, med_g, num_cells, total_reads, float(frac_on), float(frac_off), fe=fe)
    assert s2["mean_reads_per_umi_per_gene_cells_on_target"] < E.MIN_RPU_THRESHOLD
    _same_summary(s2, ref2, 0.0, low, g["e2e_is_targeted"], g["e2e_is_gex"])
    assert np.array_equal(col2, refcol2, equal_nan=True)


def test_targeted_metrics_of_a_counted_and_called_well():
    """count -> cell call -> tallies, matrix summary over the target features, statistics, fit: every number but the fit's own (checked
    above) against the restatement over the same molecules and matrix"""
    import gpu_helpers as G
    from cellranger_amd import engine as E
    from cellranger_amd import synth as S
    from cellranger_amd._lib import MS_NO_CLASS

    n = 200_000
    w = S.Workload(n_total=n, seed=S.SEED0 + 5, n_wl=100_000, n_cells=200, n_ambient=10_000, n_genes=2000)
    r = w.host_reads(0, n)
    c = G.fresh_ctx()
    c.set_whitelist(0, w.wl_packed, length=16)
    _, _, _, dev = G.gpu_barcode_stage(c, r, n)
    c.set_key_layout(w.n_genes, w.umi_len, 1, 0)
    d = [c.upload(r["umi"]), c.upload(r["umi_qualn"]), c.upload(r["feature"])]
    counts = c.count_records(c.records(n, w.umi_len, dev["idx"], d[0], d[1], d[2], dev["flags"]))
    raw = c.assemble_matrix_dev(*counts.triplets_dev(), counts.n_triplets)
    call = c.call_cells_ordmag(raw)
    assert 50 < call.n_cells < raw.n_barcodes
    is_targeted = (np.arange(w.n_genes) % 3 == 0).astype(np.uint8)
    is_gex = np.ones(w.n_genes, np.uint8)
    is_gex[::11] = 0
    tallies = counts.feature_metrics(w.n_genes, call.ranks_dev())
    mol = counts.molecules()
    exp = R.tallies(mol, w.n_genes, [0], call.ranks)
    assert all(np.array_equal(tallies[k], e) for k, e in zip(TALLY_KEYS, exp)) and exp[2].sum() > 0
    fc = np.where(is_targeted != 0, 0, MS_NO_CLASS).astype(np.uint8)
    summary = c.matrix_summary(raw, call, feature_class=fc, n_classes=1)
    s, col = E.targeted_metrics(c, tallies, is_targeted, summary, call.n_cells, n, 0.6, 0.3, is_gex=is_gex)
    rank, indptr, indices, data = raw.download()
    cells = call.cols_host().astype(np.int64)
    on = is_targeted[indices] != 0
    per_col_umis = np.add.reduceat(np.where(on, data, 0).astype(np.int64), indptr[:-1].astype(np.int64))[cells] if len(data) else np.zeros(0)
    per_col_genes = np.add.reduceat((on & (data >= 1)).astype(np.int64), indptr[:-1].astype(np.int64))[cells] if len(data) else np.zeros(0)
    empty = (indptr[1:] == indptr[:-1])[cells]
    per_col_umis[empty], per_col_genes[empty] = 0, 0
    st = E.targeted_rpu_stats(*[tallies[k] for k in TALLY_KEYS], is_targeted, is_gex)
    fe = c.rpu_gmm(st["q_value"], st["q_label"])
    ref, refcol = R.targeted_metrics(*exp, is_targeted, is_gex, np.median(per_col_umis), np.median(per_col_genes), call.n_cells, n, 0.6, 0.3, fe=fe)
    _same_summary(s, ref, 0.0, tallies, is_targeted, is_gex)
    assert np.array_equal(col, refcol, equal_nan=True) and len(col) == int(is_gex.sum())
    counts.free()
    c.close()
