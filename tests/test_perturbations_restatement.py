"""CPU checks of the restatement of MEASURE_PERTURBATIONS (tests/perturbations_numpy.py) and of engine.perturbation_clusters against it.

The grouping: hand cases written from the reference's statements (a single guide, two guides with different targets, two
Non-Targeting guides -> control, Non-Targeting plus a target -> the target, ignore_multiples, a barcode without a call by target and by
feature, a guide whose target name differs from its id, a feature reference without names).  The reference module could be loaded with
its absent dependencies stubbed (scripts/make_perturbations_golden.py), so its own outputs for these cases are recorded in
tests/golden/perturbations_reference.npz and compared as well: the partition of the cells always, numbering and names where the
reference's hash-ordered join came out sorted (in the recorded run: every case).

The draws (seed 11, stream 3, B = 4096): the mean of the bootstrap sums of a 30 %-dense vector lies within 6 standard errors of the
vector's sum (E S = sum x, Var S = n var x for n independent uniform draws), and the chi-square of the drawn index histogram against
the uniform lies below (n - 1) + 6 sqrt(2 (n - 1)), its mean plus six standard deviations."""
import os

import numpy as np
import pytest

import perturbations_numpy as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "perturbations_reference.npz")
SEED, STREAM, B = 11, 3, 4096


@pytest.mark.parametrize("case", sorted(P.HAND_CASES))
def test_grouping_hand_cases(case):
    from cellranger_amd import engine as E

    feature_ref, by_feature, ignore_multiples, want_clusters, want_names = P.HAND_CASES[case]
    for fn in (P.clusters, E.perturbation_clusters):
        per_bc, names = fn(feature_ref, P.CALLS, P.BARCODES, by_feature, ignore_multiples)
        assert per_bc.tolist() == want_clusters, fn
        assert [names[c] for c in sorted(names)] == want_names and sorted(names) == list(range(1, len(want_names) + 1)), fn
    # bytes as barcodes, as the matrix hands them over
    per_bc, _ = E.perturbation_clusters(feature_ref, P.CALLS, [b.encode() for b in P.BARCODES], by_feature, ignore_multiples)
    assert per_bc.tolist() == want_clusters


@pytest.mark.parametrize("case", sorted(P.HAND_CASES))
def test_grouping_equals_the_recorded_reference(case):
    ref = np.load(GOLDEN)
    feature_ref, by_feature, ignore_multiples, _, _ = P.HAND_CASES[case]
    per_bc, names = P.clusters(feature_ref, P.CALLS, P.BARCODES, by_feature, ignore_multiples)
    got, want = per_bc, ref[case + ".clusters"]
    assert len(got) == len(want)
    same_got, same_want = got[:, None] == got[None, :], want[:, None] == want[None, :]
    assert np.array_equal(same_got, same_want)      # the partition of the cells
    want_names = [str(n) for n in ref[case + ".names"]]
    assert sorted("|".join(sorted(n.split("|"))) for n in want_names) == sorted("|".join(sorted(n.split("|"))) for n in names.values())
    if bool(ref[case + ".sorted_join"]):
        assert got.tolist() == want.tolist() and [names[c] for c in sorted(names)] == want_names


def test_the_sorted_join_and_the_filter_list():
    # three targets in an order that is not sorted, a filtered one among them
    ref = P.FEATURE_REF + [dict(id="G9", target_gene_id="ENSG00", target_gene_name="AAA")]
    calls = {"a": ("G2|NT1|G9|G1", 4), "b": ("NT1|NT2|NT1", 3), "c": ("G9", 1)}
    per_bc, names = P.clusters(ref, calls, ["a", "b", "c", "d"])
    assert [names[c] for c in per_bc] == ["AAA|GENEA|GENEB", "Non-Targeting", "AAA", "None"]


def test_calls_from_an_assignment_matrix():
    """engine.protospacer_calls on a stand-in for MarginalCalls: CSR over the guide rows -> {barcode: (ids joined in row order, number)}"""
    from cellranger_amd import engine as E

    class Calls:
        n_rows = 3

        def assignments(self):      # guide 0: cells 0, 2; guide 1: cell 2; guide 2: cells 2, 3
            return np.array([0, 2, 3, 5], np.int64), np.array([0, 2, 2, 2, 3], np.uint32)

    calls = E.protospacer_calls(Calls(), ["G1", b"G2", "NT1"], [b"a", "b", "c", "d", "e"])
    assert calls == {"a": ("G1", 1), "c": ("G1|G2|NT1", 3), "d": ("NT1", 1)}
    per_bc, names = E.perturbation_clusters(P.FEATURE_REF, calls, ["a", "b", "c", "d", "e"])
    assert [names[c] for c in per_bc] == ["GENEA", "None", "GENEA|GENEB", "Non-Targeting", "None"]


def test_multiply_high_forms_agree():
    rs = np.random.RandomState(5)
    w = np.concatenate([rs.randint(0, 2**63, 200, dtype=np.int64).astype(np.uint64) * np.uint64(2) + np.uint64(1),
                        np.array([0, 1, 2**32 - 1, 2**32, 2**64 - 1], np.uint64)])
    for n in (1, 2, 3, 5, 257, 4097, 2**31 - 1, 2**32 - 1):
        assert P.mulhi_u64(w, n).tolist() == [P.mulhi(x, n) for x in w], n
    words = P.raw_words(SEED, STREAM, 1, 7, 9)
    assert words.dtype == np.uint64 and P.draw_indices(SEED, STREAM, 1, 7, 9).tolist() == [P.mulhi(x, 9) for x in words]
    # a draw is a prefix-stable stream: position q does not depend on n's neighbours, and sides and draws differ
    assert np.array_equal(P.raw_words(SEED, STREAM, 1, 7, 5), words[:5])
    assert not np.array_equal(P.raw_words(SEED, STREAM, 0, 7, 9), words) and not np.array_equal(P.raw_words(SEED, STREAM, 1, 8, 9), words)
    assert P.stream_id(3, 1, 7) == (3 << 33) | (1 << 32) | 7


@pytest.mark.parametrize("n", [1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 4097])
def test_bootstrap_mean_is_the_sum(n):
    rs = np.random.RandomState(100 + n)
    x = rs.randint(1, 40, n) * (rs.rand(n) < 0.3)
    S = P.bootstrap_sums(x, SEED, STREAM, 0, B).astype(np.float64)
    sigma = np.sqrt(n * x.var() / B)
    dev = abs(S.mean() - x.sum())
    print("n = %d: |mean - sum| = %.4g, sigma = %.4g" % (n, dev, sigma))
    assert dev <= 6 * sigma
    assert S.min() >= 0 and S.max() <= n * x.max()


@pytest.mark.parametrize("n", [5, 257])
def test_drawn_indices_are_uniform(n):
    hist = np.zeros(n, np.int64)
    for b in range(B):
        idx = P.draw_indices(SEED, STREAM, 0, b, n)
        assert idx.min() >= 0 and idx.max() < n
        hist += np.bincount(idx, minlength=n)
    expect = B * n / n
    chi2 = float(((hist - expect) ** 2 / expect).sum())
    print("n = %d: chi-square %.1f, bound %.1f" % (n, chi2, (n - 1) + 6 * np.sqrt(2 * (n - 1))))
    assert hist.sum() == B * n and chi2 <= (n - 1) + 6 * np.sqrt(2 * (n - 1))


def test_ci_and_summary_on_a_hand_case():
    lo, hi, fc = P.ci([3, 1, 0, 7], [1, 1, 3, 0], 1.0, 3.0, 5.0, 95.0)
    assert fc.tolist() == [np.log2(4 / 2) - np.log2(2 / 4), np.log2(2 / 2) - np.log2(2 / 4), np.log2(1 / 2) - np.log2(4 / 4), np.log2(8 / 2) - np.log2(1 / 4)]
    assert lo == np.percentile(fc, 5.0) and hi == np.percentile(fc, 95.0) and lo < hi

    # the stage around a pair test that returns fixed vectors: skip decisions, order of the rows, the raw mean, the top genes
    G, N = 6, 60
    x = np.arange(G * N).reshape(G, N) % 7
    gene_ids, gene_names = ["ENSG0%d" % g for g in range(G)], ["N%d" % (G - g) for g in range(G)]
    barcodes = ["c%d" % i for i in range(N)]
    calls = {b: ("G1", 1) for b in barcodes[:12]}
    calls.update({b: ("G2", 1) for b in barcodes[12:21]})          # 9 cells: skipped
    calls.update({b: ("NT1", 1) for b in barcodes[21:50]})
    calls.update({b: ("G1|G2", 2) for b in barcodes[50:60]})

    def compare(a, b):
        sa, sb = x[:, a].sum(axis=1), x[:, b].sum(axis=1)
        fc = np.log2((1 + sa) / (1 + sb) * len(b) / len(a))
        return dict(sums_a=sa, sums_b=sb, log2_fold_change=fc, p_values=np.full(G, 0.5), adjusted_p_values=np.linspace(0.1, 0.9, G), s_a=float(len(a)), s_b=float(len(b)))

    r = P.measure(x, gene_ids, gene_names, P.FEATURE_REF, calls, barcodes, compare, B=20, seed=2)
    assert r["names"] == ["GENEA", "GENEA|GENEB"] and r["skipped"] == ["GENEB"]
    assert r["num_cells_per_perturbation"] == {"GENEA": 12, "GENEA|GENEB": 10, "GENEB": 9, "Non-Targeting": 29}
    assert sorted(r["log2_fold_change"]["GENEA|GENEB"]) == ["GENEA", "GENEB"] and r["results_all_perturbations"].shape == (G, 6)
    assert np.array_equal(r["results_all_perturbations"][:, 0], x[:, :12].sum(axis=1) / 12)
    assert [row[2] for row in r["summary"]] == sorted(row[2] for row in r["summary"]) and len(r["summary"]) == 3
    assert r["summary_columns"][1] == "Target Gene" and r["summary"][0][6] in (10, 12) and r["summary"][0][8] == 29
    top = r["top_perturbed_genes"]["GENEA"]
    assert len(top) <= 10 and [abs(t[2]) for t in top] == sorted((abs(t[2]) for t in top), reverse=True)
    assert P.measure(x, gene_ids, gene_names, P.FEATURE_REF[:3], calls, barcodes, compare) is None                  # no Non-Targeting guide
    assert P.measure(x, gene_ids, gene_names, [dict(id="G1")], calls, barcodes, compare) is None                   # no target_gene_id
    no_control = {b: c for b, c in calls.items() if c[0] != "NT1"}
    assert P.measure(x, gene_ids, gene_names, P.FEATURE_REF, no_control, barcodes, compare) is None                 # no control cell
