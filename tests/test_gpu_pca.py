"""GPU tests of RUN_PCA on the device (crgpu_pca_dev / Context.pca / engine.run_pca, csrc/pca.hip) against tests/golden/pca_reference.npz,
which scripts/make_pca_golden.py records from the reference's own irlb.py and stats.py on the wells of tests/pca_numpy.py.

Discrete outputs (features_selected, it, mprod, the NaN pattern of the dispersion, the zero pattern of the components, the retry taken,
the components used) EQUAL the golden file.  Continuous outputs are compared after each component's sign is aligned by the sign of its
dot product with the reference's component, whose cosine must exceed 0.99 first, so that the alignment cannot hide a wrong vector.  The
bound of a fixture and quantity is 16 times the movement of the reference itself between three orders of the cells (recorded in the
golden file, floored there at 2^-53, one rounding of the largest entry), relative to the largest entry.  Nothing is fixed in advance;
every figure is printed before it is asserted.

Measured on the device (the largest over the fixtures, relative to the largest entry; bound = 16 x the reference's movement):
see the README paragraph on RUN_PCA and profiles/pca_throughput.txt."""
import numpy as np
import pytest

import pca_numpy as P

pytestmark = pytest.mark.gpu

GOLD = np.load(P.__file__.replace("pca_numpy.py", "golden/pca_reference.npz"))
WL = 1024
FACTOR = 16.0
_cache = {}


@pytest.fixture(scope="module")
def ctx():
    import gpu_helpers as G

    c = G.fresh_ctx()
    c.set_whitelist(0, np.arange(WL, dtype=np.uint32), length=16)      # rank == value: column k is barcode k
    yield c
    c.close()


def _matrix(c, dense):
    """MatrixDev of a dense features x barcodes count matrix; a barcode without counts stays as an empty column"""
    V = dense.shape[1]
    seen = np.zeros(c.n_canon, np.uint32)
    seen[:V] = 1
    c.set_counts(0, 0, seen)
    bc, ft = np.nonzero(dense.T)
    m = c.assemble_matrix_dev(c.upload(bc.astype(np.uint32)), c.upload(ft.astype(np.uint32)), c.upload(dense.T[bc, ft].astype(np.uint32)), len(bc))
    assert m.n_barcodes == V and m.nnz == len(bc)
    return m


def _run(c, name, **seams):
    from cellranger_amd import engine as E

    dense = P.FIXTURES[name]["make"]()
    m = _matrix(c, dense)
    r = E.run_pca(c, m, n_features=dense.shape[0], **P.fixture_args(name, int(GOLD[name + "_n_thresholded_bcs"])), **seams)
    m.free()
    return r


def _result(c, name):
    if name not in _cache:
        _cache[name] = _run(c, name)
    return _cache[name]


@pytest.mark.parametrize("name", sorted(P.FIXTURES))
def test_discrete_outputs_equal_the_reference(ctx, name):
    r = _result(ctx, name)
    print(name, "retried", r["retried"], "components", r["n_components"], "it", r["it"], "mprod", r["mprod"], "m_b", r["m_b"])
    assert r["retried"] == bool(GOLD[name + "_retried"])
    assert r["n_components"] == int(GOLD[name + "_n_components"])
    assert np.array_equal(r["features_selected"], GOLD[name + "_features_selected"])
    assert (r["it"], r["mprod"]) == (int(GOLD[name + "_it"]), int(GOLD[name + "_mprod"]))
    assert np.array_equal(np.isnan(r["dispersion"]), np.isnan(GOLD[name + "_dispersion"]))
    assert np.array_equal(r["components"] == 0.0, GOLD[name + "_components"] == 0.0)
    assert r["transformed_pca_matrix"].shape == GOLD[name + "_transformed"].shape and r["projection"] is r["transformed_pca_matrix"]


def _rel(got, ref):
    fin = np.isfinite(ref)
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    assert np.array_equal(got[~fin & ~np.isnan(ref)], ref[~fin & ~np.isnan(ref)])      # the infinities, with their signs
    if not fin.any():      # nothing finite to compare (every dispersion of a well NaN): the patterns above are the whole check
        return 0.0
    scale = np.abs(ref[fin]).max()
    return float(np.abs(got[fin] - ref[fin]).max() / scale)


@pytest.mark.parametrize("name", sorted(P.FIXTURES))
def test_continuous_outputs_within_the_reference_movement(ctx, name):
    r = _result(ctx, name)
    ref_c = GOLD[name + "_components"]
    signs, cos = P.align_signs(r["components"], ref_c)
    print(name, "cosines", cos.min())
    assert cos.min() > 0.99      # first: the alignment below must not hide a wrong vector
    got = dict(d=r["d"], variance_explained=r["variance_explained"], components=r["components"] * signs[:, None],
               transformed=r["transformed_pca_matrix"] * signs[None, :], dispersion=r["dispersion"])
    figures = {}
    for key, g in got.items():
        figures[key] = (_rel(g, GOLD["%s_%s" % (name, key)]), FACTOR * float(GOLD["%s_mov_%s" % (name, key)]))
        print("%-12s %-20s deviation %.3g bound %.3g" % (name, key, figures[key][0], figures[key][1]))
    for key, (dev, bound) in figures.items():
        assert dev <= bound, (name, key, dev, bound)


def _same_bits(a, b):
    for key in ("transformed_pca_matrix", "components", "variance_explained", "dispersion", "d", "features_selected"):
        assert np.array_equal(np.ascontiguousarray(a[key]).view(np.uint8), np.ascontiguousarray(b[key]).view(np.uint8)), key
    assert (a["it"], a["mprod"], a["n_components"]) == (b["it"], b["mprod"], b["n_components"])


@pytest.mark.parametrize("name", ["w257", "constructed", "feat"])
def test_bit_identical_between_runs_seams_and_start(ctx, name):
    from cellranger_amd import engine as E

    first = _result(ctx, name)
    _same_bits(first, _run(ctx, name))
    for seams in (dict(wave_block=64), dict(wave_block=128, dot_parts_per_block=3), dict(dot_parts_per_block=64)):
        _same_bits(first, _run(ctx, name, **seams))
    start = E.legacy_randn(0, first["n_used_features"])
    assert np.array_equal(start, np.random.RandomState(0).randn(first["n_used_features"]))
    _same_bits(first, _run(ctx, name, start=start))
    other = _run(ctx, name, start=np.random.RandomState(5).randn(first["n_used_features"]))      # the start is really used
    assert not np.array_equal(other["components"], first["components"])


def test_zero_count_barcode_row_is_the_centre_term(ctx):
    r = _result(ctx, "constructed")
    dense = P.FIXTURES["constructed"]["make"]()
    assert dense[:, 9].sum() == 0 and (dense[:, 7] != 0).sum() > 64 and (dense[:, 8] != 0).sum() == 1
    x, c, s = P.normalize_and_transpose(dense)
    cols = r["features_selected"]
    v = r["components"][:, cols].T
    expect = -(c / s)[cols].dot(v)
    dev = np.abs(r["transformed_pca_matrix"][9] - expect).max() / np.abs(r["transformed_pca_matrix"]).max()
    print("zero-count row: deviation %.3g" % dev)
    assert dev <= FACTOR * float(GOLD["constructed_mov_transformed"])


def _partition(labels):
    first = {}
    return np.array([first.setdefault(int(x), len(first)) for x in labels])


def test_chain_into_kmeans_gives_the_partitions_of_the_reference_projection(ctx):
    from cellranger_amd import engine as E

    dense, group = P.chain_well()
    m = _matrix(ctx, dense)
    r = E.run_pca(ctx, m, n_components=P.CHAIN["n_components"], n_features=dense.shape[0])
    m.free()
    ours = E.run_kmeans(ctx, r["projection"], max_clusters=4)
    theirs = E.run_kmeans(ctx, GOLD["chain_transformed"], max_clusters=4)
    assert sorted(ours) == sorted(theirs) and len(ours) == 3
    for key in ours:
        assert np.array_equal(_partition(ours[key]["clusters"]), _partition(theirs[key]["clusters"])), key


def test_exceptions_and_refusals_leave_the_context_usable(ctx):
    from cellranger_amd import _lib
    from cellranger_amd import engine as E

    dense = P.FIXTURES["small"]["make"]()
    m = _matrix(ctx, dense)
    with pytest.raises(E.MatrixRankTooSmall):
        ctx.pca(m, 10, min_count_threshold=2, n_features=6)
    with pytest.raises(ValueError):
        ctx.pca(m, 0, n_features=6)
    for bad in (dict(wave_block=100), dict(dot_parts_per_block=65), dict(pca_bc_indices=[3, 3]), dict(pca_bc_indices=[0, 40]), dict(start=np.zeros(5)),
                dict(start=np.array([1.0, np.nan, 0, 0, 0, 0]))):
        with pytest.raises(_lib.CrgpuError):
            ctx.pca(m, 3, n_features=6, **bad)
    with pytest.raises(_lib.CrgpuError):      # a row of the matrix beyond n_features
        ctx.pca(m, 3, n_features=5)
    r = ctx.pca(m, 10, n_features=6)      # threshold 0: reduced to the 6 features
    assert r["n_components"] == 6 and r["transformed_pca_matrix"].shape == (40, 6)
    m.free()
    empty = _matrix(ctx, np.zeros((5, 7), np.int32))
    with pytest.raises(E.NullAxisMatrix):
        E.run_pca(ctx, empty, n_components=2, n_features=5)
    empty.free()
