"""Pass A's LDS table of frequent barcodes counts the hits it answers in the free high bits of its entries' rank words
(k_lookup_hot<LH_HOTCNT>, the default of the table rounds): per-workgroup fields that wrap into VALID by device atomics,
a flush of the fields when the workgroup ends, the cold hits staged through per-wave regions.  Per-read indices after
pass A and the VALID table equal the oracle's on both whitelist sizes."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LISTS = {"737k": 737_280, "6.8m": 6_794_880}
ALL_T = 0xFFFFFFFF  # the 16-base all-T barcode: the key of an empty table slot


def _reads(w, n, giant_share, seed):
    """n reads of the workload; with giant_share, that share of them carries the cell barcode that was made all-T."""
    from cellranger_amd._lib import FLAG_CB_HAS_N

    r = w.host_reads(0, n)
    if giant_share:
        sel = np.random.default_rng(seed).random(n) < giant_share
        r["cb"][sel] = ALL_T
        r["cb_qualn"][sel] &= 0x7F                      # no N in these reads
        r["flags"][sel] &= np.uint8(~FLAG_CB_HAS_N & 0xFF)
    return r


def _pass_a_against_oracle(w, r, n):
    import gpu_helpers as G
    import oracle_lib as O
    from cellranger_amd import engine as E
    from cellranger_amd._lib import COUNTS_VALID

    c = G.fresh_ctx()
    c.set_whitelist(0, w.wl_packed, length=w.cb_len)
    _, canon_sorted = c.canon_order()
    d_cb, d_fl = c.upload(r["cb"]), c.upload(r["flags"])
    d_idx = c.empty(n, np.uint32)
    c.match_and_count(d_cb, d_fl, n, d_idx)
    idx = d_idx.to_host()
    valid = c.get_counts(0, COUNTS_VALID)
    table_rounds = c.stat(3)  # CRGPU_STAT_K1_SPLIT_ROUNDS
    c.close()
    owl = O.Whitelist(E.unpack_seqs(w.wl_packed, w.cb_len))
    res = O.run_pipeline(G.oracle_reads_from_packed(r, w.cb_len, w.umi_len), [owl], count=False, n_threads=4)
    exp_a, _ = G.oracle_expected_idx(res, canon_sorted)
    exp_valid = G.hist_as_rank_counts(res.valid_hist[0], w.cb_len, canon_sorted)
    assert np.array_equal(idx, exp_a)
    assert np.array_equal(valid, exp_valid)
    return table_rounds, valid, canon_sorted


@pytest.mark.parametrize("case", ["giant_barcode", "test_sized", "cold_regions_full"])
@pytest.mark.parametrize("wl", sorted(LISTS))
def test_table_hits_counted_in_the_table_entries(wl, case, monkeypatch):
    """giant_barcode: one cell barcode -- the all-T one, whose key is also that of an empty slot -- carries more than
    10^6 reads, so that its field wraps in every workgroup of the table round (at 4096 hits on the 737 K list, at 512 on
    the 6.8 M one).  test_sized: the cfg2 model at 600 K reads.  cold_regions_full: the per-wave regions of the cold hits
    hold 5 entries, the rest of the cold hits is counted by device atomics in the lookup."""
    from cellranger_amd import synth as S

    monkeypatch.setenv("CRGPU_HOT_MIN_READS", "1")
    n_wl = LISTS[wl]
    if case == "giant_barcode":
        n = 3_000_000 if wl == "737k" else 2_000_000
        w = S.Workload(n_total=n, seed=S.SEED0 + 41, n_wl=n_wl)
        assert not (w.wl_packed == ALL_T).any()
        w.wl_packed[w.cell_wl_pos[0]] = ALL_T           # (the generator reads the list through a pointer)
        r = _reads(w, n, 0.6, 43)
    else:
        n = 600_000
        if case == "cold_regions_full":
            monkeypatch.setenv("CRGPU_COLD_CAP", "5")
        w = S.Workload(n_total=n, seed=S.SEED0 + 42, n_wl=n_wl)
        r = _reads(w, n, 0.0, 0)
    rounds, valid, canon_sorted = _pass_a_against_oracle(w, r, n)
    assert rounds >= 1
    if case == "giant_barcode":
        giant = int(np.searchsorted(canon_sorted, np.uint32(ALL_T)))
        assert canon_sorted[giant] == ALL_T and valid[giant] > 1_000_000
