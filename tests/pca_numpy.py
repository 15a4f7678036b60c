"""The wells of the RUN_PCA tests and a numpy restatement of the stage (no GPU, no reference tree).

FIXTURES maps a name to what scripts/make_pca_golden.py records and the tests replay: a seeded count matrix (features x barcodes, the
orientation of CountMatrix.m) and the arguments of run_pca.  The matrices are built here, by numpy's legacy RandomState, so the golden
file holds results only.

run_pca(matrix, ...) restates lib/python/cellranger/analysis/pca.py:49-209 with normalize_and_transpose, analysis/stats.py
(normalize_by_umi, summarize_columns with scikit-learn 1.7.2's mean_variance_axis formula, get_normalized_dispersion) and
analysis/irlb.py:61-231 in plain numpy on dense arrays, with a selectable order of the cells in every sum over cells (`cell_order`:
None, or a permutation applied to the cells before the sums and undone on the outputs).  The SVD of B is numpy's, so the signs of the
components are LAPACK's here; the device states its own rule (include/crgpu.h) and the tests align signs before they compare."""
import numpy as np

TOL, MAXIT = 1e-4, 50
DEFAULT_RUNPCA_THRESHOLD = 2


class MatrixRankTooSmall(Exception):
    pass


class NullAxisMatrix(Exception):
    pass


# ---- the wells ------------------------------------------------------------------------------------------------------------------
def grouped_well(seed, n_cells, n_features, n_groups=3, depth=400.0):
    """cells of n_groups expression profiles, Poisson counts, log-normal depths -> int32 [features x cells]"""
    rs = np.random.RandomState(seed)
    prof = rs.gamma(0.6, 1.0, size=(n_groups, n_features)) + 0.02
    for g in range(n_groups):      # a block of marker features per group
        lo = (g * n_features) // (2 * n_groups)
        prof[g, lo:lo + max(2, n_features // (4 * n_groups))] *= 6.0 + 2.0 * g
    prof /= prof.sum(axis=1, keepdims=True)
    group = rs.randint(0, n_groups, size=n_cells)
    d = depth * np.exp(rs.normal(0.0, 0.35, size=n_cells))
    return rs.poisson(prof[group] * d[:, None]).T.astype(np.int32), group


def threshold_well(seed):
    """grouped, then barcodes and features pushed to sums of 0, 1 and 2: the threshold 2 removes them, org_cols_used is no identity"""
    m, _ = grouped_well(seed, 150, 90, depth=300.0)
    m[:, [3, 70, 149]] = 0
    m[5, 3], m[5, 70], m[6, 70] = 1, 1, 1          # barcode sums 1 and 2
    m[[0, 17, 44, 89], :] = 0
    m[17, 10], m[44, 11], m[44, 12] = 1, 1, 1      # feature sums 1 and 2
    m[60, :] = 0
    m[60, 3] = 2                                   # a feature whose counts sit on a removed barcode only
    return m


def small_well(seed):
    """6 features x 40 barcodes for 10 components: too small a rank at threshold 2, 6 components at threshold 0"""
    rs = np.random.RandomState(seed)
    base = np.array([[30, 2, 9, 1, 14, 5], [3, 25, 2, 12, 4, 16]])
    return rs.poisson(base[rs.randint(0, 2, size=40)] * np.exp(rs.normal(0, 0.3, size=(40, 1)))).T.astype(np.int32) + 1


def constructed_well(seed):
    """grouped 120 x 80, then: barcode 7 with 100 entries of 120 features (more than a wave), barcode 8 with one entry, barcode 9 empty"""
    m, _ = grouped_well(seed, 80, 120, depth=60.0)
    m[:100, 7] = np.maximum(m[:100, 7], 1)
    m[100:, 7] = 0
    m[:, 8] = 0
    m[31, 8] = 5
    m[:, 9] = 0
    return m


def equal_depth_well(seed, n_cells=96, n_features=60):
    """every cell has the same depth, so every factor is 1.0: a grouped well, a filler feature that tops each cell up to the deepest
    one, and a last feature that holds 3 in every cell: log2(1 + 3) = 2 exactly, its mean is 2 and its variance exactly 0 in any order"""
    m, _ = grouped_well(seed, n_cells, n_features, depth=4000.0)      # deep: no two features share a multiset of counts
    depth = m.sum(axis=0)
    m = np.vstack([m, (depth.max() + 5 - depth)[None, :], np.full((1, n_cells), 3)]).astype(np.int32)
    assert len(set(m.sum(axis=0))) == 1
    return m


def mad_zero_well(seed):
    """grouped 80 x 120, then 40 copies of one feature: they fill a bin of means, its MAD is 0, the copies' dispersion is 0 / 0 and
    the rest of the bin +- inf"""
    m, _ = grouped_well(seed, 120, 80, depth=250.0)
    m[40:80, :] = m[39, :]
    return m


def equal_means_well(seed, n=36, swaps=30000):
    """every row sum and every column sum equal: 3 x 3 blocks of equal margins (a feature group high in its own cell group), a circulant
    on top, then seeded 2 x 2 swaps that keep both margins.  All depths equal (the factors are 1.0) and all means equal, bit for bit:
    get_normalized_dispersion returns the raw dispersion"""
    rs = np.random.RandomState(seed)
    base = rs.multinomial(400, rs.dirichlet(np.full(n, 0.5)))
    size = n // 3
    m = np.array([np.roll(base, f) for f in range(n)], dtype=np.int64)
    blocks = np.array([[6, 1, 2], [1, 5, 3], [2, 3, 4]])      # equal margins, three distinct eigenvalues
    m += np.kron(blocks, np.ones((size, size), dtype=np.int64))
    for _ in range(swaps):
        a, b, c, d = rs.randint(0, n, size=4)
        if a != b and c != d and m[a, d] > 0 and m[b, c] > 0:
            m[a, c] += 1
            m[b, d] += 1
            m[a, d] -= 1
            m[b, c] -= 1
    assert len(set(m.sum(axis=0))) == 1 and len(set(m.sum(axis=1))) == 1
    return m.astype(np.int32)


FIXTURES = {
    "w257": dict(make=lambda: grouped_well(11, 257, 130)[0], n_components=5),
    "w300": dict(make=lambda: grouped_well(12, 300, 200)[0], n_components=10),
    "w700": dict(make=lambda: grouped_well(13, 700, 500, n_groups=4)[0], n_components=20),
    "thr": dict(make=lambda: threshold_well(14), n_components=5),
    "small": dict(make=lambda: small_well(15), n_components=10),
    "constructed": dict(make=lambda: constructed_well(16), n_components=4),
    "var0": dict(make=lambda: equal_depth_well(17), n_components=3),
    "mad0": dict(make=lambda: mad_zero_well(18), n_components=4),
    "equal": dict(make=lambda: equal_means_well(19), n_components=3),
    "feat": dict(make=lambda: grouped_well(12, 300, 200)[0], n_components=10, pca_features=120),
    "bcs": dict(make=lambda: grouped_well(11, 257, 130)[0], n_components=5, pca_bc_step=2),
}
CHAIN = dict(seed=21, n_cells=240, n_features=150, n_components=6, n_clusters=3)


def chain_well():
    return grouped_well(CHAIN["seed"], CHAIN["n_cells"], CHAIN["n_features"], depth=900.0)


def fixture_args(name, n_thresholded_bcs=None):
    """-> the keyword arguments of run_pca / engine.run_pca for a fixture; pca_bc_step needs the thresholded barcode count"""
    f = FIXTURES[name]
    kw = dict(n_components=f["n_components"], pca_features=f.get("pca_features"))
    if "pca_bc_step" in f and n_thresholded_bcs is not None:
        kw["pca_bc_indices"] = np.arange(0, n_thresholded_bcs, f["pca_bc_step"])
    return kw


# ---- stats.py -------------------------------------------------------------------------------------------------------------------
def threshold_axes(m, threshold):
    """select_axes_above_threshold: barcodes first, then the features of what is left"""
    bcs = np.flatnonzero(m.sum(axis=0) > threshold)
    feats = np.flatnonzero(m[:, bcs].sum(axis=1) > threshold)
    if len(bcs) == 0 or len(feats) == 0:
        raise NullAxisMatrix()
    return bcs, feats


def normalize_by_umi(m):
    counts = m.sum(axis=0)
    med = max(1.0, np.median(counts))
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(m != 0, m.astype(np.float64) * (med / counts)[None, :], 0.0)


def mean_variance(x, counts):
    """mean_variance_axis of scikit-learn 1.7.2 over the cells (axis 1 here) of the entries with counts != 0, left to right"""
    n = x.shape[1]
    nz = counts != 0
    nnz = nz.sum(axis=1)
    mean = np.zeros(x.shape[0])
    for c in range(n):
        mean += np.where(nz[:, c], x[:, c], 0.0)
    mean /= n
    corr, var = np.zeros(x.shape[0]), np.zeros(x.shape[0])
    for c in range(n):
        diff = np.where(nz[:, c], x[:, c] - mean, 0.0)
        corr += diff
        var += diff * diff
    some = nnz != n
    corr = np.where(some, corr - (n - nnz) * mean, corr)
    corr = corr ** 2 / n
    var = np.where(some, var + (n - nnz) * mean ** 2, var)
    return mean, (var - corr) / n


def binned_median(x, values, edges):
    """scipy.stats.binned_statistic(x, values, "median", bins=edges): left-closed bins, the last one closed on both sides -> the
    medians (NaN for an empty bin) and the bin numbers from 1"""
    b = np.digitize(x, edges)
    b[x == edges[-1]] = len(edges) - 1
    med = np.full(len(edges) - 1, np.nan)
    for i in range(1, len(edges)):
        v = values[b == i]
        if len(v):
            med[i - 1] = np.median(v)
    return med, b


def normalized_dispersion(mu, var, nbins=20):
    with np.errstate(divide="ignore", invalid="ignore"):
        disp = (var - mu) / np.square(mu)
        q = np.percentile(mu, np.arange(0, 100, 100 // nbins))
        q = np.unique(np.append(q, mu.max()))
        if len(q) <= 1:
            return disp
        meds, bins = binned_median(mu, disp, q)
        meds_arr = meds[bins - 1]
        mads, bins = binned_median(mu, np.abs(disp - meds_arr), q)
        return (disp - meds_arr) / mads[bins - 1]


# ---- irlb.py --------------------------------------------------------------------------------------------------------------------
def irlb(a, nu, center, start, record=None):
    """irlb(A, nu, center=center) on the dense cells x features a, statement by statement; start: the unnormalised first vector"""
    eps2 = 2 * np.finfo(float).eps

    def invcheck(x):
        return 1.0 / x if x > eps2 else 0.0

    m, n = a.shape
    if min(m, n) < 2:
        raise ValueError("The input matrix must be at least 2x2.")
    m_b = min(nu + 20, 3 * nu, min(a.shape))
    mprod = it = j = 0
    k, smax = nu, 1
    V, W, B = np.zeros((n, m_b)), np.zeros((m, m_b)), np.zeros((m_b, m_b))
    V[:, 0] = start
    V[:, 0] = V[:, 0] / np.linalg.norm(V)
    while it < MAXIT:
        if it > 0:
            j = k
        W[:, j] = a.dot(V[:, j]) - np.dot(center, V[:, j])
        mprod += 1
        if it > 0:
            W[:, j] = W[:, j] - W[:, 0:j].dot(W[:, j].dot(W[:, 0:j]))
        s = np.linalg.norm(W[:, j])
        W[:, j] = invcheck(s) * W[:, j]
        while j < m_b:
            F = a.T.dot(W[:, j])
            mprod += 1
            F = F - np.sum(W[:, j]) * center
            F = F - s * V[:, j]
            F = F - V[:, 0:j + 1].dot(F.dot(V[:, 0:j + 1]))
            fn = np.linalg.norm(F)
            F = invcheck(fn) * F
            if j < m_b - 1:
                V[:, j + 1] = F
                B[j, j], B[j, j + 1] = s, fn
                W[:, j + 1] = a.dot(V[:, j + 1]) - np.dot(center, V[:, j + 1])
                mprod += 1
                W[:, j + 1] = W[:, j + 1] - fn * W[:, j]
                W[:, j + 1] = W[:, j + 1] - W[:, 0:j + 1].dot(W[:, j + 1].dot(W[:, 0:j + 1]))
                s = np.linalg.norm(W[:, j + 1])
                W[:, j + 1] = invcheck(s) * W[:, j + 1]
            else:
                B[j, j] = s
            j += 1
        S = np.linalg.svd(B)
        R = fn * S[0][m_b - 1, :]
        smax = S[1][0] if it < 1 else max(S[1][0], smax)
        if record is not None:
            record.append(dict(B=B.copy(), R=R.copy(), smax=smax))
        conv = int(np.sum(np.abs(R[0:nu]) < TOL * smax))
        if conv >= nu:
            break
        k = min(max(conv + nu, k), m_b - 3)
        V[:, 0:k] = V[:, 0:m_b].dot(S[2].T[:, 0:k])
        V[:, k] = F
        B = np.zeros((m_b, m_b))
        B[np.arange(k), np.arange(k)] = S[1][:k]
        B[0:k, k] = R[0:k]
        W[:, 0:k] = W[:, 0:m_b].dot(S[0][:, 0:k])
        it += 1
    return S[1][0:nu], V[:, 0:m_b].dot(S[2].T[:, 0:nu]), it, mprod


# ---- pca.py ---------------------------------------------------------------------------------------------------------------------
def normalize_and_transpose(m):
    x = normalize_by_umi(m)
    with np.errstate(invalid="ignore"):
        x = np.where(m != 0, np.log2(1 + x), 0.0)
    c, v = mean_variance(x, m)
    v[v == 0.0] = 1.0
    return x.T, c, np.sqrt(v)


def run_pca(matrix, n_components=10, pca_features=None, pca_bc_indices=None, seed=0, min_count_threshold=0, cell_order=None, record=None):
    """-> dict(transformed_pca_matrix, components, variance_explained, dispersion, features_selected (indices), d, it, mprod, mu, var,
    n_components).  cell_order permutes the barcodes of `matrix` first and puts the rows of the projection back"""
    matrix = np.asarray(matrix)
    if cell_order is not None:
        assert pca_bc_indices is None
        matrix = matrix[:, cell_order]
    bcs, feats = threshold_axes(matrix, min_count_threshold)
    thr = matrix[np.ix_(feats, bcs)]
    if pca_bc_indices is None:
        pca_bc_indices = np.arange(len(bcs))
    pca_bc_indices = np.asarray(pca_bc_indices)
    n_feat = len(feats) if pca_features is None else min(int(pca_features), len(feats))
    mu, var = mean_variance(normalize_by_umi(thr), thr)
    dispersion = normalized_dispersion(mu, var)
    order = np.argsort(dispersion, kind="stable")[-n_feat:]
    rank = min(n_feat, len(pca_bc_indices))
    if rank < n_components:
        if min_count_threshold == DEFAULT_RUNPCA_THRESHOLD:
            raise MatrixRankTooSmall("Matrix rank is too small")
        n_components = rank
    pca_mat = thr[np.ix_(order, pca_bc_indices)]
    x, c, s = normalize_and_transpose(pca_mat)
    x = x * (1.0 / s)[None, :]
    c = c / s
    d, v, it, mprod = irlb(x, n_components, c, np.random.RandomState(seed).randn(len(order)), record)
    fx, fc, fs = normalize_and_transpose(matrix)
    fx = fx * (1.0 / fs)[None, :]
    cols = feats[order]
    transformed = fx[:, cols].dot(v) - (fc / fs)[cols].dot(v)
    components = np.zeros((n_components, matrix.shape[0]))
    components[:, cols] = v.T
    full_disp = np.full(matrix.shape[0], np.nan)
    full_disp[feats] = dispersion
    if cell_order is not None:
        back = np.empty_like(cell_order)
        back[cell_order] = np.arange(len(cell_order))
        transformed = transformed[back]
    return dict(transformed_pca_matrix=transformed, components=components,
                variance_explained=np.square(d) / ((len(pca_bc_indices) - 1) * len(order)), dispersion=full_disp, features_selected=cols,
                d=d, it=it, mprod=mprod, mu=mu, var=var, n_components=n_components, n_thresholded_bcs=len(bcs))


def run_stage(matrix, **kw):
    """the retry of the stage: threshold 2, then 0 -> (result, retried)"""
    try:
        return run_pca(matrix, min_count_threshold=DEFAULT_RUNPCA_THRESHOLD, **kw), False
    except (NullAxisMatrix, MatrixRankTooSmall):
        return run_pca(matrix, min_count_threshold=0, **kw), True


def align_signs(got_components, ref_components):
    """-> (signs, |cosines|): per component the sign of its dot product with the reference's and the cosine's magnitude"""
    dots = np.einsum("ij,ij->i", got_components, ref_components)
    norms = np.linalg.norm(got_components, axis=1) * np.linalg.norm(ref_components, axis=1)
    return np.where(dots < 0, -1.0, 1.0), np.abs(dots) / norms
