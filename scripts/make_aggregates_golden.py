"""Record the reference's own outputs for the aggregate fixtures of tests/aggregates_numpy.py.

    python scripts/make_aggregates_golden.py <reference>/lib/python

Imports the reference's cellranger.feature.antibody.analysis (nothing of it is copied) and runs detect_aggregate_barcodes,
detect_outlier_umis_bcs, detect_highly_corrected_bcs, _calculate_fraction_to_use and the read-fraction columns of the correction
table on every fixture of golden_fixtures(), through a duck-typed matrix object.  Only RESULTS go into
tests/golden/aggregates_reference.npz: column indices, thresholds, the summed read fractions.

The reference sorts with numpy's default (unstable) sort, so which of several equal values at the K-th place it takes is not
specified.  Every fixture is therefore required to be tie-insensitive: the restatement must give the same columns under the tie rules
"high" and "low".  The script stops otherwise, and it stops when the reference disagrees with the restatement.
"""
import os
import sys

import numpy as np
import pandas as pd
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import aggregates_numpy as R  # noqa: E402

TYPE_OF_KIND = {R.KIND_OTHER: "Gene Expression", R.KIND_ANTIBODY: R.AB, R.KIND_ANTIGEN: R.AG}


class _Def:
    def __init__(self, i, feature_type):
        self.id, self.feature_type = "F%04d" % i, feature_type


class _Ref:
    def __init__(self, defs):
        self.feature_defs = defs


class DuckMatrix:
    """what the three functions touch of a CountMatrix: m, bcs, feature_ref.feature_defs, select_features_by_type, get_counts_per_bc,
    select_barcodes"""

    def __init__(self, m, bcs, defs):
        self.m, self.bcs, self.feature_ref = m, bcs, _Ref(defs)

    def select_features_by_type(self, feature_type):
        keep = [i for i, d in enumerate(self.feature_ref.feature_defs) if d.feature_type == feature_type]
        return DuckMatrix(self.m[keep, :], self.bcs, [self.feature_ref.feature_defs[i] for i in keep])

    def get_counts_per_bc(self):
        return np.asarray(self.m.sum(axis=0)).ravel()

    def select_barcodes(self, idx):
        idx = list(idx)
        return DuckMatrix(self.m[:, idx], [self.bcs[i] for i in idx], self.feature_ref.feature_defs)


def duck(fx):
    V = len(fx["indptr"]) - 1
    m = sp.csc_matrix((fx["data"].astype(np.int64), fx["indices"], fx["indptr"]), shape=(fx["n_features"], V))
    return DuckMatrix(m, ["BC%08d-1" % c for c in range(V)], [_Def(i, TYPE_OF_KIND[int(k)]) for i, k in enumerate(fx["kind"])])


def cols_of(bcs):
    return np.array(sorted(int(b[2:10]) for b in bcs), np.uint64)


def main(ref_python):
    sys.path.insert(0, ref_python)
    import cellranger.feature.antibody.analysis as A

    out = {"fraction_n": np.arange(5, 65), "fraction": np.array([A._calculate_fraction_to_use(n) for n in range(5, 65)])}
    n_nonempty = 0
    for name, fx in R.golden_fixtures():
        hi, lo = R.remove_aggregates(fx, "high"), R.remove_aggregates(fx, "low")
        assert np.array_equal(hi["removed"], lo["removed"]) and np.array_equal(hi["reasons"], lo["reasons"]), "%s is tie-sensitive" % name
        mat = duck(fx)
        agg = cols_of(A.detect_aggregate_barcodes(mat, num_probe_barcodes=fx["num_probe_barcodes"]))
        outl = cols_of(A.detect_outlier_umis_bcs(mat))
        V = len(mat.bcs)
        table = pd.concat([pd.DataFrame({"barcode": mat.bcs, "library_type": lib, "reads": fx["reads"][lib],
                                         "umi_corrected_reads": fx["corrected"].get(lib, np.zeros(V, np.int64)),
                                         "candidate_dup_reads": np.zeros(V, np.int64)}) for lib in (R.AB, R.AG)], ignore_index=True)
        A.augment_correction_table_with_corrected_reads_fraction(table)
        A.augment_correction_table_with_read_fraction(table)
        ab_table = A.filter_correction_table(table, R.AB)
        high = cols_of(A.detect_highly_corrected_bcs(ab_table))
        ab_removed = list(set(high.tolist()) | set(agg.tolist()))      # the union, in the order a Python set gives
        lost_ab = A.subselect_augmented_table([mat.bcs[c] for c in ab_removed], ab_table)[A.FRACTION_TOTAL_READS].sum()
        ag_table = A.filter_correction_table(table, R.AG)
        lost_ag = A.subselect_augmented_table([mat.bcs[int(c)] for c in outl], ag_table)[A.FRACTION_TOTAL_READS].sum()
        # the reference and the restatement agree
        assert np.array_equal(agg, hi["removed"][(hi["reasons"] & R.COUNTS) != 0]), name
        assert np.array_equal(outl, hi["removed"][(hi["reasons"] & R.ANTIGEN) != 0]), name
        assert np.array_equal(high, hi["removed"][(hi["reasons"] & R.HIGHLY_CORRECTED) != 0]), name
        n_nonempty += len(agg) > 0
        out.update({name + "/aggregates": agg, name + "/outliers": outl, name + "/highly_corrected": high,
                    name + "/reads_lost": np.array([lost_ab, lost_ag], np.float64)})
        print("%s: V %d, %d signal antibodies, K %d: %d aggregates, %d highly corrected, %d antigen outliers" % (
            name, V, hi["info"]["n_signal"], hi["info"]["top_k"], len(agg), len(high), len(outl)))
    assert n_nonempty >= 4, "too few fixtures with an aggregate"
    path = os.path.join(ROOT, "tests", "golden", "aggregates_reference.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
