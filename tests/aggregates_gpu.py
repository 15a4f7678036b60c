"""What the GPU tests of the aggregate stage and of the closing cell filters share: contexts created under a given CRGPU_AGG_LDS_ROWS
(read when a context is created) and device matrices of the fixtures of tests/aggregates_numpy.py, built as
tests/test_gpu_matrix_summary.py::_matrix builds them: column k is whitelist entry k."""
import os

import numpy as np

WL = 4096
_ctxs = {}


def ctx(lds=None):
    """the context of this setting (None: the variable unset), made once"""
    import gpu_helpers as G

    if lds not in _ctxs:
        old = os.environ.pop("CRGPU_AGG_LDS_ROWS", None)
        try:
            if lds is not None:
                os.environ["CRGPU_AGG_LDS_ROWS"] = lds
            c = G.fresh_ctx()
        finally:
            os.environ.pop("CRGPU_AGG_LDS_ROWS", None)
            if old is not None:
                os.environ["CRGPU_AGG_LDS_ROWS"] = old
        c.set_whitelist(0, np.arange(WL, dtype=np.uint32), length=16)      # rank == value: column k is barcode k
        _ctxs[lds] = c
    return _ctxs[lds]


def matrix(c, fx):
    indptr, V = fx["indptr"], len(fx["indptr"]) - 1
    seen = np.zeros(c.n_canon, np.uint32)
    seen[:V] = 1
    c.set_counts(0, 0, seen)
    c.set_counts(0, 1, np.zeros(len(seen), np.uint32))
    bc = np.repeat(np.arange(V, dtype=np.uint32), np.diff(indptr))
    m = c.assemble_matrix_dev(c.upload(bc), c.upload(fx["indices"].astype(np.uint32)), c.upload(fx["data"].astype(np.uint32)), len(bc))
    assert m.n_barcodes == V and m.nnz == len(bc)
    return m
