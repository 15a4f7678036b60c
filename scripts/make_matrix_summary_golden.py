#!/usr/bin/env python
"""Record the reference's own outputs of the masked sums behind the filtered-matrix summary -> tests/golden/matrix_summary_reference.npz.

    python scripts/make_matrix_summary_golden.py <reference checkout>/lib/python

Needs the reference's Python package on the given path (cellranger.sparse is imported from it; nothing of it is copied) and scipy, so
it runs only where that checkout exists; the tests read the recorded file.  cellranger.rna.report_matrix itself needs h5py and the
pipeline's own modules and is not imported: the glue between the recorded functions (which mask goes with which metric, the order
statistics, the top features) is tests/matrix_summary_numpy.py, which tests/test_matrix_summary_restatement.py then pins against
what is recorded here.

For every fixture of matrix_summary_numpy.golden_fixtures() and every class k, three views are recorded, all with the class's
features as row mask: the class's own cells ("own"), every listed cell ("union") and every column ("all").  Of each view:
sum_masked with axis 0, 1 and None, count_ge_masked with thresholds 1 and 2 and axis 0, 1 and None.  The reference's row sums are
int32 (scipy keeps the matrix's dtype): the fixtures stay below 2^31 there.  Results only: a few KB."""
import os
import sys

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import matrix_summary_numpy as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "matrix_summary_reference.npz")


def views(fx):
    """(name, row mask, column mask) of every recorded view"""
    V = len(fx["indptr"]) - 1
    cells = fx["cells"].astype(np.int64)
    listed = np.zeros(V, bool)
    listed[cells] = True
    for k in range(fx["n_classes"]):
        rows = fx["feature_class"] == k
        own = np.zeros(V, bool)
        own[cells[((fx["cell_class_mask"] >> np.uint32(k)) & 1).astype(bool)]] = True
        for name, cols in (("own", own), ("union", listed), ("all", np.ones(V, bool))):
            yield "c%d_%s" % (k, name), rows, cols


def main(ref_path):
    sys.path.insert(0, ref_path)
    import cellranger.sparse as cr_sparse

    out = {}
    for fname, fx in R.golden_fixtures().items():
        V = len(fx["indptr"]) - 1
        m = sp.csc_matrix((fx["data"], fx["indices"], fx["indptr"].astype(np.int32)), shape=(fx["n_features"], V))
        for vname, rows, cols in views(fx):
            key = "%s_%s" % (fname, vname)
            for axis, tag in ((0, "0"), (1, "1"), (None, "n")):
                s = cr_sparse.sum_masked(m, rows, cols, axis)
                assert np.all(np.asarray(s) >= 0)      # no int32 wrap in the reference
                out["%s_sum_%s" % (key, tag)] = np.asarray(s).astype(np.int64)
                for thr in (1, 2):
                    c = cr_sparse.count_ge_masked(m, rows, cols, thr, axis)
                    out["%s_ge%d_%s" % (key, thr, tag)] = np.asarray(c).astype(np.int64)
    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    print("%d arrays, %d bytes -> %s" % (len(out), size, OUT))
    assert size < 256 * 1024


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
