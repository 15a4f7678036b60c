"""Host checks of the constructed ingest cases (tests/ingest_cases.py): every case has the structure it claims, the FASTQ
restatement refuses every refusal case, and the restatements agree with one another where they overlap -- pack on slices of
FASTQ rows against pack_rows on the rows, the tiled reference of the large text against the restatement run over all of
it, the oracle's shard metrics against a dict-based reading of make_shard_metrics.rs:263-332 -- on exactly the inputs the
device is compared on (tests/test_gpu_ingest_edges.py)."""
import numpy as np
import pytest

import ingest_cases as IC


# ---- a second reading of the shard metrics ------------------------------------------------------------------------------------
def py_shard_metrics(cb, cbq, umi, uq, hit=None):
    """plain Python over the ASCII reads: the counters of MakeShardVisitor::visit_processed_read for the barcode and UMI parts"""
    m = dict.fromkeys(("sequenced_reads", "bc_n_bases", "bc_bases", "umi_n_bases", "umi_bases", "bc_q30_bases", "bc_q30_den",
                       "umi_q30_bases", "umi_q30_den", "good_umi", "has_n_barcode", "has_n_umi", "homopolymer_barcode",
                       "homopolymer_umi", "low_min_qual_barcode", "low_min_qual_umi", "miss_whitelist_barcode", "polyt_suffix_umi"), 0)
    for r in range(len(cb)):
        b, bq, u, q = cb[r].tobytes(), cbq[r].tobytes(), umi[r].tobytes(), uq[r].tobytes()
        m["sequenced_reads"] += 1
        for part, s, ql in (("bc", b, bq), ("umi", u, q)):
            m[part + "_n_bases"] += s.count(b"N")
            m[part + "_bases"] += len(s)
            m[part + "_q30_den"] += sum(1 for x in ql if x > 35)
            m[part + "_q30_bases"] += sum(1 for x in ql if x > 35 and x >= 63)
        homo = {k: len(set(s)) == 1 for k, s in (("b", b), ("u", u))}
        low = any((x - 33) % 256 < 10 for x in q)
        m["good_umi"] += not (b"N" in u or homo["u"] or low)
        m["has_n_barcode"] += b"N" in b
        m["has_n_umi"] += b"N" in u
        m["homopolymer_barcode"] += homo["b"]
        m["homopolymer_umi"] += homo["u"]
        m["low_min_qual_barcode"] += (min(bq) - 33) % 256 < 10
        m["low_min_qual_umi"] += (min(q) - 33) % 256 < 10
        if hit is not None:
            m["miss_whitelist_barcode"] += not hit[r]
        if len(u) >= 5:
            m["polyt_suffix_umi"] += u.endswith(b"TTTTT")
    return m


# ---- tests ----------------------------------------------------------------------------------------------------------------------
def test_constants_come_from_the_source():
    assert IC.FQ_TILE % 256 == 0 and IC.THREAD_WRAP == 524288 and IC.WAVE_WRAP == 8192
    assert IC.fastq_plan(1) == (1, 1, 256) and IC.fastq_plan(4 * IC.FQ_TILE) == (1, 1, 4 * IC.FQ_TILE)
    assert IC.fastq_plan(4 * IC.FQ_TILE + 1)[:2] == (2, 2)
    assert IC.fastq_plan(4096 * 4 * IC.FQ_TILE + 1)[0] == 4096 and IC.fastq_plan(4096 * 4 * IC.FQ_TILE + 1)[2] > 4 * IC.FQ_TILE
    with pytest.raises(RuntimeError):
        IC._need("tile = tile / 2;", r"tile\s*=\s*\(tile\s*\+\s*255\)", "the rounding")
    from cellranger_amd._lib import FLAG_CB_HAS_N, MISS

    assert IC.FLAG_CB_HAS_N == FLAG_CB_HAS_N and IC.MISS == MISS


@pytest.mark.parametrize("case", IC.small_fastq_cases(), ids=lambda c: c.name)
def test_small_fastq_case_has_the_structure_it_claims(case):
    d = IC.check_small_case(case)
    seq, qual, lens = IC.fastq_rows(case.text, case.stride)        # accepted
    assert len(lens) * 4 == d["n_lines"] and lens.tolist() == d["seq_lens"]
    for r, L in enumerate(lens):
        assert not seq[r, min(L, case.stride):].any() and not qual[r, min(L, case.stride):].any()
        assert (seq[r, :min(L, case.stride)] != 0).all()


def test_small_fastq_cases_cover_the_list():
    names = [c.name for c in IC.small_fastq_cases()]
    assert len(set(names)) == len(names)
    for stride in (1, 63, 64, 65, 100, 200):
        assert "stride_%d_lf" % stride in names
    # line ends do not change the rows
    by = {c.name: c for c in IC.small_fastq_cases()}
    for a, b in (("one_lf", "one_crlf"), ("one_lf", "one_lf_nofinal"), ("one_lf", "one_crlf_nofinal"), ("one_lf", "one_crlf_ends_in_cr"),
                 ("trap_lf", "trap_crlf_nofinal"), ("stride_64_lf", "stride_64_crlf"), ("empty_reads_lf", "empty_reads_crlf")):
        for x, y in zip(IC.fastq_rows(by[a].text, 64), IC.fastq_rows(by[b].text, 64)):
            assert np.array_equal(x, y), (a, b)


@pytest.mark.parametrize("variant", list(IC.SWEEP_VARIANTS))
def test_sweep_hits_every_boundary(variant):
    ev = IC.check_sweep(variant)
    assert not ev["len_one_more"]          # the plan takes the tile from the length: see one_byte_tile_text
    ref = IC.fastq_rows(IC.sweep_text(variant, 0), IC.SWEEP_STRIDE)
    assert ref[2].max() > IC.SWEEP_STRIDE and ref[2].min() == 0
    for d in (1, 255, 256, IC.SWEEP_D - 1):                        # the padding of the first header moves no row
        for x, y in zip(IC.fastq_rows(IC.sweep_text(variant, d), IC.SWEEP_STRIDE), ref):
            assert np.array_equal(x, y)
        assert len(IC.sweep_text(variant, d)) == len(IC.sweep_text(variant, 0)) + d


def test_text_with_a_tile_of_one_byte():
    text = IC.one_byte_tile_text()
    d = IC.describe_text(text)
    assert d["len_mod_tile"] == 1 and d["nb"] >= 2 and d["final_lf"] and d["n_lines"] % 4 == 0
    assert (d["nb"] - 1) * d["tile"] + 1 == d["n_bytes"]


def test_large_text_and_its_tiled_reference():
    case = IC.large_fastq_case()
    IC.check_large_case(case)
    seq, qual, lens = IC.fastq_rows(case.text.tobytes(), case.stride)   # the restatement over all of the text
    assert np.array_equal(seq, case.seq) and np.array_equal(qual, case.qual) and np.array_equal(lens, case.lens)
    assert len(lens) == case.n > IC.WAVE_WRAP


def test_wrap_case():
    case = IC.wrap_fastq_case()
    IC.check_small_case(case)
    assert case.n == IC.WAVE_WRAP + 5


def test_every_refusal_case_is_refused_by_the_restatement():
    cases, base, n_good = IC.refusal_cases()
    names = set(c.name for c in cases)
    assert {"lines_4k+1", "lines_4k+2", "lines_4k+3", "header_without_at_first", "header_without_at_middle", "header_without_at_last",
            "separator_without_plus", "quality_one_short_last", "line_feeds_only"} <= names
    for c in cases:
        IC.check_refusal_case(c)
    assert len(IC.fastq_rows(base, 8)[2]) == n_good                # the text they were made from is accepted
    assert len(IC.fastq_rows(b"", 8)[2]) == 0


def test_pack_on_slices_of_fastq_rows_equals_pack_rows():
    seq, qual, lens = IC.fastq_rows(IC.sweep_text("lf", 0), IC.SWEEP_STRIDE)
    for off, L in ((0, 16), (16, 12), (1, 1), (IC.SWEEP_STRIDE - 16, 16), (7, 5)):
        a = IC.pack_ref(np.ascontiguousarray(seq[:, off:off + L]), np.ascontiguousarray(qual[:, off:off + L]))
        b = IC.pack_rows_ref(seq, qual, off, L)
        for x, y in zip(a, b):
            assert np.array_equal(x, y)
        # and pack_rows_var with whole reads is pack_rows
        k, qn, ln = IC.pack_rows_var_ref(seq, qual, np.full(len(seq), IC.SWEEP_STRIDE, np.uint32), off, L, 1)
        assert np.array_equal(k, a[0]) and np.array_equal(qn, a[1]) and (ln == L).all()
    # the zero padding of short reads packs as N
    short = lens < 16
    assert short.any() and IC.pack_rows_ref(seq, qual, 0, 16)[2][short].all()


def test_pack_restatement_by_hand():
    k, qn, has_n = IC.pack_ref(np.frombuffer(b"ACGTaN.T", np.uint8).reshape(2, 4), np.array([[33, 127, 128, 255], [0, 73, 200, 126]], np.uint8))
    assert k.tolist() == [0b00011011, 0b00000011] and has_n.tolist() == [False, True]
    assert qn.tolist() == [[33, 127, 127, 127], [0x80, 73 | 0x80, 127 | 0x80, 126]]
    seq, qual = IC.byte_value_blocks(5, "base")
    assert IC.pack_ref(seq, qual)[2].sum() == 5 * 252
    # the formula above k_pack_rows_var, by hand: 3' v3 UMIs (offset 16, 12 bases, at least 10)
    rows = np.frombuffer(b"ACGT" * 10, np.uint8).reshape(1, 40).repeat(6, 0)
    _, qn, ln = IC.pack_rows_var_ref(rows, rows, np.array([40, 28, 27, 26, 25, 0], np.uint32), 16, 12, 10)
    assert ln.tolist() == [12, 12, 11, 10, 0, 0] and not qn[2, 11:].any() and qn[2, 10] != 0 and not qn[4].any()
    for off, length, mn in IC.pack_var_triples():
        assert off + length <= IC.PACK_VAR_STRIDE and 1 <= mn <= length


@pytest.mark.parametrize("lens", [(16, 12), (1, 1), (5, 4)])
def test_oracle_shard_metrics_equal_the_dict_restatement(lens):
    import oracle_lib as O

    cb, cbq, umi, uq, classes = IC.shard_reads(*lens)
    idx = IC.shard_idx(len(cb))
    hit = (idx != IC.MISS).astype(np.uint8)
    assert O.shard_metrics(cb, cbq, umi, uq, hit) == py_shard_metrics(cb, cbq, umi, uq, hit)
    exp = O.shard_metrics(cb, cbq, umi, uq)
    assert exp == py_shard_metrics(cb, cbq, umi, uq)
    assert exp["sequenced_reads"] == len(cb) and exp["miss_whitelist_barcode"] == 0
    if lens == (16, 12):
        assert exp["polyt_suffix_umi"] >= 3 and exp["homopolymer_umi"] >= 5 and exp["low_min_qual_umi"] > 12


def test_shard_case_with_counters_at_zero():
    import oracle_lib as O

    exp = O.shard_metrics(*IC.shard_zero_reads(), exact_hit=np.ones(300, np.uint8))
    assert all(exp[f] == 0 for f in IC.SHARD_ZERO_FIELDS) and exp["good_umi"] == 300 == exp["sequenced_reads"]


@pytest.mark.parametrize("run_len", IC.HP_RUN_LENS)
def test_homopolymer_cases_have_the_structure_they_claim(run_len):
    for exact_end in (False, True):
        case = IC.hp_positive_case(run_len, exact_end)
        IC.check_hp_positive(case)
        assert IC.homopolymer_ref(case.rows, case.lens, case.stride, run_len) == case.expect
    case = IC.hp_near_miss_case(run_len)
    IC.check_hp_near_miss(case)
    assert IC.homopolymer_ref(case.rows, case.lens, case.stride, run_len) == case.expect
    rows, lens, stride, exp = IC.hp_edge_rows(run_len)
    assert IC.homopolymer_ref(rows, lens, stride, run_len) == exp


def test_rows_metrics_restatement_by_hand():
    seq = np.frombuffer(b"NNACnN..", np.uint8).reshape(2, 4)
    qual = np.array([[35, 36, 62, 63], [255, 0, 33, 73]], np.uint8)
    assert IC.rows_metrics_ref(seq, qual, np.array([4, 2], np.uint32), 4) == dict(n_bases=3, bases=6, q30_bases=2, q30_den=4)
    assert IC.rows_metrics_ref(seq, qual, None, 4) == dict(n_bases=3, bases=8, q30_bases=3, q30_den=5)
    s, q, lens = IC.rows_metrics_rows()
    assert set(IC.ROWS_LENGTHS) <= set(lens.tolist()) and IC.ROWS_STRIDE in lens and lens.max() > IC.ROWS_STRIDE
    r1, l1, r2, l2 = IC.hp_pair_case()
    assert IC.homopolymer_ref(r1, l1, r1.shape[1], 15) == dict(A=4, C=2, G=2, T=2)
    assert IC.homopolymer_ref(r1, l1, r1.shape[1], 15, r2, l2, r2.shape[1]) == dict(A=6, C=3, G=3, T=3)
