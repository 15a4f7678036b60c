"""Multiplexed Flex wells on the device against the restatement tests/rtl_tags_numpy.py: the tag of every column, barcodes and UMIs
per tag, the columns of every sample, the gel-bead overlaps with and without the antibody part, the medians per probe barcode, the
GEM occupancy and the high-occupancy-GEM removal.  Every comparison is equality; f64 values are compared as bit patterns with NaN
equal to NaN.  Matrices are built as tests/test_gpu_emptydrops.py::_matrix builds them: set_barcode_segments, set_counts,
assemble_matrix_dev."""
import numpy as np
import pytest

import gpu_helpers as G
import rtl_tags_numpy as R
from cellranger_amd import _lib
from cellranger_amd import engine as E

pytestmark = pytest.mark.gpu

GEX, AB = "Gene Expression", R.ANTIBODY
NONE64 = 0xFFFFFFFFFFFFFFFF
_ctxs = {}


def _ctx(n_gel, n_probe):
    """one context per construct: gel beads 0 .. n_gel - 1 as 16-mers, probe barcodes 0 .. n_probe - 1 as 8-mers"""
    if (n_gel, n_probe) not in _ctxs:
        c = G.fresh_ctx(dense=False)
        c.set_barcode_segments(0, [np.arange(n_gel, dtype=np.uint32), np.arange(n_probe, dtype=np.uint32)], [16, 8])
        _ctxs[(n_gel, n_probe)] = c
    return _ctxs[(n_gel, n_probe)]


class Well:
    """ranks: ascending canonical ranks of the columns; counts: {feature: count} per column"""

    def __init__(self, n_gel, n_probe, ranks, counts, feature_type):
        self.c, self.n_probe = _ctx(n_gel, n_probe), n_probe
        self.ranks = np.asarray(ranks, np.uint32)
        self.counts, self.feature_type = counts, feature_type
        self.cols = [(int(r) // n_probe, int(r) % n_probe) for r in self.ranks]
        c = self.c
        seen = np.zeros(c.n_canon, np.uint32)
        seen[self.ranks] = 1
        c.set_counts(0, 0, seen)
        bc = np.array([r for r, col in zip(self.ranks, counts) for _ in col], np.uint32)
        ft = np.array([f for col in counts for f in sorted(col)], np.uint32)
        ct = np.array([col[f] for col in counts for f in sorted(col)], np.uint32)
        self.m = c.assemble_matrix_dev(c.upload(bc), c.upload(ft), c.upload(ct), len(bc))
        assert self.m.n_barcodes == len(self.ranks) and self.m.nnz == len(bc)

    def call(self, cells):
        cells = np.ascontiguousarray(cells, dtype=np.uint64)
        c = self.c
        return E.CellCall(c, c.upload(cells) if len(cells) else c.empty(0, np.uint64), len(cells), {"filtered_bcs": len(cells)}, self.m)


def _random_well(seed, n_gel, n_probe, V, n_features=6, types=(GEX,), consecutive_from=None, max_count=40):
    rng = np.random.RandomState(seed)
    if consecutive_from is None:
        ranks = np.sort(rng.choice(n_gel * n_probe, V, replace=False))
    else:
        ranks = np.arange(consecutive_from, consecutive_from + V)
    feature_type = [types[f % len(types)] for f in range(n_features)]
    counts = []
    for _ in range(V):
        k = rng.randint(0, 4)
        counts.append({int(f): int(rng.randint(1, max_count)) for f in rng.choice(n_features, k, replace=False)})
    return Well(n_gel, n_probe, ranks, counts, feature_type)


def _ids(n):
    return ["BC%03d" % (k + 1) for k in range(n)]


def _bits_equal(a, b):
    return (np.isnan(a) and np.isnan(b)) or np.float64(a).view(np.uint64) == np.float64(b).view(np.uint64)


def _same_rows(got, ref):
    assert len(got) == len(ref)
    for g, r in zip(got, ref):
        assert (g["barcode1_id"], g["barcode2_id"], g["barcode1_gems"], g["barcode2_gems"], g["common_gems"]) == r[:5]
        assert _bits_equal(g["overlap"], r[5])


def _check_stage(w, cells, probe_ids, pairings=None):
    """engine.call_tags_rtl, the occupancy outputs and the medians against the restatement"""
    c, cells = w.c, [int(x) for x in cells]
    out = E.call_tags_rtl(c, w.m, w.call(cells), probe_ids, w.feature_type, {GEX: None, AB: "ANTIBODY"}, pairings)
    per_tag, rows, metrics, umi = R.call_tags_rtl(w.cols, w.counts, w.feature_type, probe_ids, cells, pairings)
    ids, tag = out["tag_ids"], {i: t for t, i in enumerate(out["tag_ids"])}
    assert np.array_equal(out["tags"].tags, np.array([tag[probe_ids[p]] for _, p in w.cols], np.uint8))
    assert out["barcodes_per_tag"] == {i: len(v) for i, v in per_tag.items()}
    _same_rows(out["rows"], rows)
    m = out["metrics"]
    assert m["filtered_gel_bead_barcodes_count"] == metrics["filtered_gel_bead_barcodes_count"]
    assert m["filtered_barcodes_per_probe_barcode"] == metrics["filtered_barcodes_per_probe_barcode"]
    assert set(m["probe_barcode_overlap_coefficients"]) == set(metrics["probe_barcode_overlap_coefficients"])
    for k, v in metrics["probe_barcode_overlap_coefficients"].items():
        assert _bits_equal(m["probe_barcode_overlap_coefficients"][k], v)
    for ty, name in ((GEX, "umi_per_probe_barcode"), (AB, "ANTIBODY_umi_per_probe_barcode")):
        if ty in w.feature_type:
            assert m[name] == umi.get(ty, {})
    # occupancy
    runs = out["runs"]
    cc = [w.cols[k] for k in cells]
    assert runs.n_cells == len(cells) and runs.n_gems == len(set(g for g, _ in w.cols))
    cpp, first = np.zeros(w.n_probe, np.uint64), np.full(w.n_probe, NONE64, np.uint64)
    for k in cells:
        p = w.cols[k][1]
        cpp[p] += 1
        first[p] = min(int(first[p]), k)
    assert np.array_equal(runs.cells_per_probe, cpp) and np.array_equal(runs.first_cell_col_per_probe, first)
    cells_per_tag = np.zeros(len(ids), np.uint64)
    for _, p in cc:
        cells_per_tag[tag[probe_ids[p]]] += 1
    assert np.array_equal(runs.cells_per_tag, cells_per_tag)
    if cells:
        hist, lam, probes, per_gem = R.occupancy(cc)
        got = E.rtl_occupancy_summary(runs.cells_per_gem_hist, runs.gems_with_cells, runs.cells_per_probe)
        assert runs.gems_with_cells == len(per_gem) and got["histogram"] == hist and got["total_probe_barcodes"] == probes
        assert _bits_equal(got["estimated_lambda"], lam)
    else:
        assert runs.gems_with_cells == 0 and not runs.cells_per_gem_hist.any()
    # medians of every feature type
    ref_med = R.median_umi_per_cell(w.cols, w.counts, w.feature_type, cells)
    for ty in dict.fromkeys(w.feature_type):
        sums = c.column_sums(w.m, np.array([t == ty for t in w.feature_type]))
        nz, med = c.rtl_medians(sums, w.call(cells))
        for p in range(w.n_probe):
            vals = [sum(n for f, n in w.counts[k].items() if w.feature_type[f] == ty) for k in cells if w.cols[k][1] == p]
            vals = [v for v in vals if v > 0]
            assert nz[p] == len(vals)
            assert (int(med[p]) if vals else None) == ref_med.get((ty, p))
    return out


def _check_removal(w, cells, thr):
    cells = [int(x) for x in cells]
    kept, n_high, n_in, f_gems, f_cells = R.remove_high_occupancy([w.cols[k] for k in cells], thr)
    call, d = w.c.remove_high_occupancy_gems(w.m, w.call(cells), thr)
    assert call.cols_host().tolist() == [cells[k] for k in kept] and call.n_cells == len(kept) == d["n_kept"]
    assert (d["high_occupancy_gems"], d["cells_in_high_occupancy_gems"], d["n_cells"], d["threshold"]) == (n_high, n_in, len(cells), thr)
    assert _bits_equal(d["fraction_cell_gems_high_occupancy"], f_gems) and _bits_equal(d["fraction_cells_in_high_occupancy_gems"], f_cells)
    return call


# ---- the smallest wells ----------------------------------------------------------------------------------------------------------
def test_no_column_one_column_no_cell_and_empty_columns():
    ft = [GEX]
    w0 = Well(50, 3, [], [], ft)                                          # V = 0
    out = _check_stage(w0, [], _ids(3))
    assert out["rows"] == [] and out["barcodes_per_tag"] == {}
    _check_removal(w0, [], 1)
    w1 = Well(50, 3, [7], [{0: 5}], ft)                                   # V = 1
    _check_stage(w1, [0], _ids(3))
    _check_stage(w1, [], _ids(3))                                         # no cells
    _check_removal(w1, [0], 0)
    we = Well(50, 3, [3, 4, 5, 9, 10], [{}] * 5, ft)                      # all columns empty: they still carry a tag and can be cells
    out = _check_stage(we, [0, 1, 2, 4], _ids(3))
    assert out["barcodes_per_tag"] == {"BC001": 2, "BC002": 2, "BC003": 1} and out["metrics"]["umi_per_probe_barcode"] == {}


def test_the_hand_well_of_the_restatement_tests():
    import test_rtl_tags_restatement as H

    w = Well(50, 3, [g * 3 + p for g, p in H.W5], [{0: 1}] * len(H.W5), [GEX])
    out = _check_stage(w, range(len(H.W5)), H.IDS3)
    assert [r["overlap"] for r in out["rows"]] == [2 / 3, 0.5, 1.0] and out["metrics"]["filtered_gel_bead_barcodes_count"] == 5
    assert _check_removal(w, range(len(H.W5)), 1).cols_host().tolist() == [2, 8]
    for thr in (0, 3):
        _check_removal(w, range(len(H.W5)), thr)


@pytest.mark.parametrize("n_probe,n_ids", [(1, 1), (3, 3), (16, 16), (16, 1), (64, 64)])
def test_probe_and_tag_counts(n_probe, n_ids):
    """n_probe 1, 3, 16; 1, 16 and 64 tags -- with 64 the last tag uses bit 63 of a run's mask"""
    w = _random_well(11 + n_probe + n_ids, 40, n_probe, min(400, 30 * n_probe))
    ids = _ids(n_ids)
    probe_ids = [ids[p % n_ids] for p in range(n_probe)]
    rng = np.random.RandomState(5)
    cells = np.flatnonzero(rng.rand(len(w.ranks)) < 0.5)
    out = _check_stage(w, cells, probe_ids)
    if n_ids == 64:
        assert out["runs"].present[63] and out["runs"].common[:, 63].sum() > 0
    for thr in (0, 1, n_probe):
        _check_removal(w, cells, thr)


def test_a_probe_rank_that_is_not_on_the_map():
    w = Well(20, 4, [0, 1, 2, 4, 5, 9], [{0: 1}] * 6, [GEX])             # probe rank 3 is never used
    ids = ["BC001", "BC002", "BC003", None]
    out = E.call_tags_rtl(w.c, w.m, w.call([0, 1, 3]), ids, w.feature_type)
    assert out["barcodes_per_tag"] == {"BC001": 2, "BC002": 3, "BC003": 1}
    bad = ["BC001", None, "BC003", "BC004"]                               # probe rank 1 is used by columns 1, 4 and 5
    with pytest.raises(E.CrgpuError) as e:
        E.call_tags_rtl(w.c, w.m, w.call([0]), bad, w.feature_type)
    assert e.value.code == -1


def test_two_probe_ranks_of_one_tag_in_one_gem_count_once():
    w = Well(20, 3, [21, 22, 26], [{0: 2}] * 3, [GEX])                    # GEM 7: probes 0 and 1; GEM 8: probe 2
    out = _check_stage(w, [0, 1, 2], ["BC001", "BC001", "BC002"])
    assert out["runs"].gems_per_tag.tolist() == [1, 1] and out["runs"].cells_per_tag.tolist() == [2, 1]
    assert out["metrics"]["filtered_barcodes_per_probe_barcode"] == {"BC001": 1, "BC002": 1}


@pytest.mark.parametrize("V", [255, 256, 257])
def test_full_runs_across_tile_and_wave_boundaries(V):
    """consecutive ranks from 5 with 16 probes: runs of all 16 probes begin at columns 11, 27, ...: one spans columns 59 .. 74 (a
    wave boundary), one 251 .. 266 (columns 255 / 256 / 257 of a workgroup's tile, cut short by V)"""
    w = _random_well(V, 40, 16, V, consecutive_from=5)
    _check_stage(w, range(V), _ids(16))                                    # every column a cell
    rng = np.random.RandomState(V)
    cells = np.flatnonzero(rng.rand(V) < 0.3)
    _check_stage(w, cells, _ids(16))
    w2 = _random_well(V + 1, 40, 16, 300, consecutive_from=5)              # the run 251 .. 266 complete
    out = _check_stage(w2, range(300), _ids(16))
    assert out["runs"].cells_per_gem_hist[16] == 18                       # ranks 16 .. 303
    _check_removal(w2, range(300), 15)


def test_more_than_one_grid_pass():
    """65 537 columns: 257 workgroups, the last one with a single column; the cell list spans several tiles of the compaction"""
    V = 65537
    w = _random_well(3, 5000, 16, V, n_features=4, consecutive_from=3)
    rng = np.random.RandomState(1)
    cells = np.flatnonzero(rng.rand(V) < 0.2)
    _check_stage(w, cells, _ids(16))
    _check_removal(w, cells, 4)


def test_umi_sum_above_32_bits():
    big = 2 ** 31 - 1
    w = Well(20, 2, [0, 2, 4, 5], [{0: big, 1: big}, {0: big}, {0: big}, {1: 7}], [GEX, AB])
    out = _check_stage(w, [0, 3], ["BC001", "BC002"])
    assert out["metrics"]["umi_per_probe_barcode"]["BC001"] == 3 * big > 2 ** 32
    assert out["metrics"]["ANTIBODY_umi_per_probe_barcode"] == {"BC001": big, "BC002": 7}
    bad_ft = np.zeros(1, np.uint8)                                         # the matrix holds row 1
    with pytest.raises(E.CrgpuError) as e:
        w.c.rtl_tags(w.m, [0, 1], 2, bad_ft, 1)
    assert e.value.code == -1


# ---- the antibody part -------------------------------------------------------------------------------------------------------------
def test_antibody_pairings_of_the_hand_case():
    import test_rtl_tags_restatement as H

    w = Well(20, 2, [g * 2 + p for g, p in H.AB_COLS], H.AB_COUNTS, H.AB_TYPES)
    out = _check_stage(w, H.AB_CELLS, H.AB_IDS, H.AB_PAIRS)
    assert [(r["barcode1_id"], r["barcode2_id"], r["overlap"]) for r in out["rows"]] == [
        ("BC001", "BC002", 1.0), ("BC001", "AB002", 0.5), ("BC002", "AB001", 1.0)]
    counts = [{0: 5}, {0: 3, 1: 100}, {1: 3}, {1: 10}, {0: 7}, {1: 2}]     # AB001 is removed: no cell of probe 0 holds Antibody counts
    w = Well(20, 2, [g * 2 + p for g, p in H.AB_COLS], counts, H.AB_TYPES)
    out = _check_stage(w, H.AB_CELLS, H.AB_IDS, H.AB_PAIRS)
    assert [(r["barcode1_id"], r["barcode2_id"]) for r in out["rows"]] == [("BC001", "BC002"), ("BC001", "AB002")]


def _combined(w, cells, tag_of_probe, ab_tag_of_probe, low, n_tags):
    """the combined map of detect_suspicious_rtl_ab_pairings for given thresholds (None = removed), keyed by tag"""
    ab = {}
    for (gel, p), col in zip(w.cols, w.counts):
        n = sum(v for f, v in col.items() if w.feature_type[f] == AB)
        if n:
            per = ab.setdefault(ab_tag_of_probe[p], {})
            per[gel] = per.get(gel, 0) + n
    comb = {t: {g: n for g, n in per.items() if n >= low[t]} for t, per in ab.items() if low[t] is not None}
    for k in cells:
        gel, p = w.cols[k]
        per = comb.setdefault(tag_of_probe[p], {})
        per[gel] = per.get(gel, 0) + 1
    return comb


def test_antibody_thresholds_removed_zero_all_dropped_and_split_sums():
    # three probe ranks: 0 -> tag 0 (RTL side), 1 and 2 -> their Antibody counts both go to tag 2; tag 3 has counts and is removed
    ft = [GEX, AB]
    cols = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 0), (2, 1), (3, 2), (4, 3), (5, 0)]
    counts = [{0: 9, 1: 4}, {1: 6}, {1: 5}, {1: 6}, {}, {0: 2}, {1: 20}, {1: 3}, {1: 50}, {0: 1, 1: 1}]
    w = Well(20, 4, [g * 4 + p for g, p in cols], counts, ft)
    cells = [0, 5]
    top, abt = [0, 1, 1, 3], [1, 2, 2, 3]
    tags = w.c.rtl_tags(w.m, top, 4)
    sums = w.c.column_sums(w.m, np.array([False, True]))
    for low in ([1, 11, 11, None],        # GEM 0: 6 + 5 = 11 reaches 11 only together; GEM 1: 6 alone does not; GEM 2: 20 does
                [0, 0, 0, 0],             # a threshold of 0 keeps every GEM with a count, and none without
                [5, None, 1000, None],    # tag 2 keeps its key and loses every entry: 0 GEMs, NaN overlaps
                [None, None, None, None]):
        ref = _combined(w, cells, top, abt, low, 4)
        runs = w.c.rtl_gem_runs(w.m, tags, w.call(cells), ab=(abt, sums, [NONE64 if x is None else x for x in low]))
        assert runs.present.tolist() == [t in ref for t in range(4)]
        assert runs.gems_per_tag.tolist() == [len(ref.get(t, {})) for t in range(4)]
        rows = E.rtl_overlap_rows(runs.gems_per_tag, runs.common, runs.present)
        ref_rows = R.overlap_rows(ref)
        assert len(rows) == len(ref_rows)
        for g, r in zip(rows, ref_rows):
            assert (g["tag1"], g["tag2"], g["gems1"], g["gems2"], g["common_gems"]) == r[:5] and _bits_equal(g["overlap"], r[5])
        if low[2] == 11:
            assert runs.gems_per_tag[2] == 2 and set(ref[2]) == {0, 2}
        if low[2] == 1000:
            assert runs.gems_per_tag[2] == 0 and runs.present[2] and all(np.isnan(g["overlap"]) for g in rows if 2 in (g["tag1"], g["tag2"]))
    off = w.c.rtl_gem_runs(w.m, tags, w.call(cells))                       # the antibody part off: the filtered matrix alone
    assert off.present.tolist() == [True, False, False, False] and off.gems_per_tag.tolist() == [2, 0, 0, 0]


# ---- the columns of every sample ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_samples", [1, 17])
def test_sample_columns_equal_a_stable_partition(n_samples):
    n_probe = 24
    w = _random_well(40 + n_samples, 60, n_probe, 1200)
    tags = w.c.rtl_tags(w.m, np.arange(n_probe), n_probe)
    rng = np.random.RandomState(n_samples)
    sot = rng.randint(0, n_samples, n_probe).astype(np.uint8)
    sot[[2, 11]] = 0xFF                                                    # tags without a sample
    host_tags = np.array([p for _, p in w.cols])
    cells = np.flatnonzero(rng.rand(len(w.ranks)) < 0.4)
    for cols in (None, cells, np.zeros(0, np.uint64)):
        base = np.arange(len(w.ranks)) if cols is None else np.asarray(cols, np.int64)
        s = sot[host_tags[base]] if len(base) else np.zeros(0, np.uint8)
        want = [base[s == k] for k in range(n_samples)]
        d, off = tags.sample_columns(sot, n_samples, None if cols is None else w.call(cols))
        assert off.tolist() == np.concatenate([[0], np.cumsum([len(x) for x in want])]).tolist()
        assert d.to_host(int(off[-1])).tolist() == np.concatenate(want).tolist() if len(base) else int(off[-1]) == 0
    d, off = tags.sample_columns(np.full(n_probe, 0xFF, np.uint8), n_samples)      # no tag has a sample: nothing is allocated
    assert not off.any() and d.size == 0
    with pytest.raises(ValueError):
        w.c.rtl_tags(w.m, np.arange(n_probe - 1), n_probe)                         # one entry per probe rank


def test_medians_per_probe_even_odd_single_and_none():
    """four probe ranks, by hand: probe 0 has the cell sums 3 9 4 8 -> sorted 3 4 8 9, (4 + 8) / 2 = 6; probe 1 has 7 2 5 -> 5;
    probe 2 has one cell with 11; probe 3 has a cell with sum 0 and a column with 50 that is no cell: no value.  An even count
    whose middle sum is odd rounds down: the cells with 9 and 4 alone give (4 + 9) / 2 = 6."""
    cols = [(0, 0), (0, 1), (0, 3), (1, 0), (1, 1), (2, 0), (2, 1), (2, 2), (3, 0), (3, 3)]
    sums = [3, 7, 0, 9, 2, 4, 5, 11, 8, 50]
    w = Well(20, 4, [g * 4 + p for g, p in cols], [{0: s} if s else {} for s in sums], [GEX])
    d_sums = w.c.column_sums(w.m)
    assert d_sums.to_host().tolist() == sums
    nz, med = w.c.rtl_medians(d_sums, w.call([0, 1, 2, 3, 4, 5, 6, 7, 8]))
    assert nz.tolist() == [4, 3, 1, 0] and med.tolist() == [6, 5, 11, 0]
    nz, med = w.c.rtl_medians(d_sums, w.call([0, 3, 5]))
    assert nz.tolist() == [3, 0, 0, 0] and med.tolist() == [4, 0, 0, 0]
    nz, med = w.c.rtl_medians(d_sums, w.call([3, 5]))
    assert nz.tolist() == [2, 0, 0, 0] and med.tolist() == [6, 0, 0, 0]          # (4 + 9) / 2 = 6 in integers
    nz, med = w.c.rtl_medians(d_sums, w.call([]))
    assert not nz.any() and not med.any()


# ---- a 16-plex well end to end -----------------------------------------------------------------------------------------------------
def test_sixteen_plex_well_end_to_end():
    V, n_probe, n_samples = 20000, 16, 4
    w = _random_well(77, 3000, n_probe, V, n_features=8, types=(GEX, GEX, GEX, AB))
    rng = np.random.RandomState(9)
    cells = np.flatnonzero(rng.rand(V) < 0.15)
    ids = _ids(n_probe)
    out = _check_stage(w, cells, ids)
    runs = out["runs"]
    occ = E.rtl_occupancy_summary(runs.cells_per_gem_hist, runs.gems_with_cells, runs.cells_per_probe)
    thr = E.high_occupancy_gem_threshold(occ["estimated_lambda"], runs.cells_per_probe, runs.first_cell_col_per_probe, 200000)
    assert thr == R.threshold(occ["estimated_lambda"], [w.cols[k][1] for k in cells], 200000) >= 1
    kept = _check_removal(w, cells, thr)
    _check_removal(w, cells, 1)
    # the per-sample filtered matrices equal numpy slicing of the downloaded matrix
    sot = (np.arange(n_probe) % n_samples).astype(np.uint8)
    d_cols, off = out["tags"].sample_columns(sot, n_samples, kept)
    rank, indptr, indices, data = w.m.download()
    kept_h = kept.cols_host()
    for s in range(n_samples):
        n = int(off[s + 1] - off[s])
        want_cols = kept_h[sot[[w.cols[k][1] for k in kept_h]] == s]
        assert n == len(want_cols) > 0
        mv = E.C.POINTER(_lib.MatrixDevView)()
        w.c._check(w.c.L.crgpu_select_barcodes_cols_dev(w.c.h, w.m._mv, E.C.c_void_p(d_cols.ptr + 8 * int(off[s])), n, E.C.byref(mv)))
        r2, p2, i2, d2 = E.MatrixDev(w.c, mv).download()
        assert np.array_equal(r2, rank[want_cols])
        assert np.array_equal(np.diff(p2), np.diff(indptr)[want_cols])
        pick = np.concatenate([np.arange(indptr[k], indptr[k + 1]) for k in want_cols])
        assert np.array_equal(i2, indices[pick]) and np.array_equal(d2, data[pick])
        d_ranks = w.c.empty(n, np.uint32)
        w.c._check(w.c.L.crgpu_cell_ranks_dev(w.c.h, w.m._mv, E.C.c_void_p(d_cols.ptr + 8 * int(off[s])), n, E._p(d_ranks)))
        assert np.array_equal(d_ranks.to_host(n), rank[want_cols])


def test_probe_matrix_accepts_the_sample_ranks():
    """the ranks of one sample's cells are what crgpu_assemble_probe_matrix_dev takes as d_sample_ranks"""
    n_gel, n_probe, n_feat, LU, n = 300, 4, 5, 8, 4000
    c = G.fresh_ctx(dense=False)
    c.set_barcode_segments(0, [np.arange(n_gel, dtype=np.uint32), np.arange(n_probe, dtype=np.uint32)], [16, 8])
    rng = np.random.RandomState(2)
    idx = rng.randint(0, n_gel * n_probe, n).astype(np.uint32)
    seen = np.bincount(idx, minlength=n_gel * n_probe).astype(np.uint32)
    c.set_counts(0, 0, seen)
    c.set_key_layout(n_feat, LU, 1, 0)
    gene = rng.randint(0, n_feat, n).astype(np.uint32)
    probe = rng.randint(0, 3 * n_feat, n).astype(np.int32)
    d_um, d_uq = c.upload(rng.randint(0, 1 << 16, n).astype(np.uint32)), c.upload(np.full((n, LU), 40, np.uint8))
    counts = c.count_records(c.records(n, LU, c.upload(idx), d_um, d_uq, c.upload(gene), c.zeros(n, np.uint8), d_probe_idx=c.upload(probe)))
    t = counts.triplets()
    m = c.assemble_matrix_dev(c.upload(t[0].astype(np.uint32)), c.upload(t[1].astype(np.uint32)), c.upload(t[2].astype(np.uint32)), len(t[0]))
    rank = m.download()[0]
    cells = np.flatnonzero(rng.rand(m.n_barcodes) < 0.5).astype(np.uint64)
    call = E.CellCall(c, c.upload(cells), len(cells), {"filtered_bcs": len(cells)}, m)
    tags = c.rtl_tags(m, np.arange(n_probe), n_probe)
    d_cols, off = tags.sample_columns([0, 1, 0xFF, 1], 2, call)
    lo, hi = int(off[1]), int(off[2])
    want = np.array([k for k in cells if rank[k] % n_probe in (1, 3)], np.uint64)
    assert d_cols.to_host(int(off[-1]))[lo:hi].tolist() == want.tolist() and hi > lo
    d_ranks = c.empty(hi - lo, np.uint32)
    c._check(c.L.crgpu_cell_ranks_dev(c.h, m._mv, E.C.c_void_p(d_cols.ptr + 8 * lo), hi - lo, E._p(d_ranks)))
    pm = counts.probe_matrix(3 * n_feat, d_ranks)
    assert pm.n_barcodes == hi - lo and np.array_equal(pm.download()[0], rank[want.astype(np.int64)])
    c.close()
