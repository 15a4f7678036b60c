"""numpy restatement of RUN_KMEANS: scikit-learn 1.7.2's KMeans(n_clusters, random_state) -- centring, tolerance, k-means++ seeding,
Lloyd with the relocation of empty clusters, inertia -- and the reference's compute_db_index and relabel_by_size (cellranger's
analysis/kmeans.py and clustering.py cannot be imported without numexpr, so both are restated and pinned by hand-computed cases in
tests/test_kmeans_restatement.py).  Nothing here is copied from either; it is the arithmetic the device code (csrc/kmeans.h)
follows, with every sum over cells (the per-cluster sums of a round, the per-cluster wss, the inertia) taken in one of three orders so
that the recorder can measure how far a sum order moves a result.

Also the fixtures of the golden file: `FIXTURES` names them and `fixture_data(name)` regenerates their matrices from seeds, so that
tests/golden/kmeans_reference.npz holds recorded RESULTS only."""
import math

import numpy as np

ORDERS = ("cell", "partial256", "reverse")
MIN_CENTROID_DIST = 1e-3


# ---- the random stream -------------------------------------------------------------------------------------------------------------------
def trials(k):
    return 2 + int(np.log(k))


def seed_draws(seed, n, k):
    """the doubles the seeding consumes, in order, and the first cell (choice(n, p = 1 / n))"""
    rs = np.random.RandomState(seed)
    u = rs.random_sample(1 + (k - 1) * trials(k))
    p = np.full(n, 1.0) / float(n)
    cdf = np.cumsum(p)
    cdf /= cdf[-1]
    return u, int(min(np.searchsorted(cdf, u[0], side="right"), n - 1))


# ---- steps 1 - 3 -------------------------------------------------------------------------------------------------------------------------
def center(X):
    X = np.asarray(X, dtype=np.float64)
    mean = np.add.reduce(X, axis=0) / X.shape[0]      # rows in row order
    Xc = X - mean
    xx = np.zeros(len(Xc))
    for t in range(Xc.shape[1]):      # dimension order
        xx += Xc[:, t] * Xc[:, t]
    return Xc, mean, xx


def tolerance(X, factor=1e-4):
    return 0.0 if factor == 0 else float(np.mean(np.var(np.asarray(X, dtype=np.float64), axis=0)) * factor)


def _seed_dist(Xc, xx, idx):
    """euclidean_distances(X[idx], X, squared): ((-2 x.y) + ||y||^2) + ||x||^2, not below 0 -> [len(idx), n]"""
    dots = np.zeros((len(idx), len(Xc)))
    for t in range(Xc.shape[1]):
        dots += Xc[idx, t][:, None] * Xc[None, :, t]
    return np.maximum((-2.0 * dots + xx[idx][:, None]) + xx[None, :], 0.0)


def kmeans_plusplus(Xc, xx, k, u, first, diag=None):
    """-> the indices of the k seeds.  diag (a dict) receives the smallest relative distance of a draw to a boundary of the
    cumulative sum and of the winning potential to the runner-up"""
    n, T = len(Xc), trials(k)
    idx = [first]
    closest = _seed_dist(Xc, xx, [first])[0]
    pot = float(np.cumsum(closest)[-1])
    for c in range(1, k):
        vals = u[1 + (c - 1) * T: 1 + c * T] * pot
        cum = np.cumsum(closest)
        cand = np.minimum(np.searchsorted(cum, vals), n - 1)
        dist = np.minimum(closest[None, :], _seed_dist(Xc, xx, cand))
        pots = np.array([np.cumsum(r)[-1] for r in dist])
        best = int(np.argmin(pots))
        if diag is not None and pot > 0:
            for v, ci in zip(vals, cand):
                edges = [cum[ci]] + ([cum[ci - 1]] if ci else [])
                diag["draw"] = min([diag.get("draw", np.inf)] + [abs(v - e) / pot for e in edges])
            for j in range(T):      # equal rows have equal potentials in every arithmetic, and the first wins in all of them
                if not np.array_equal(Xc[cand[j]], Xc[cand[best]]):
                    diag["pot"] = min(diag.get("pot", np.inf), abs(pots[j] - pots[best]) / max(pots[best], 1e-300))
        pot, closest = float(pots[best]), dist[best]
        idx.append(int(cand[best]))
    return np.array(idx, dtype=np.int64)


# ---- step 5 --------------------------------------------------------------------------------------------------------------------------------
def _ordered_sum(v, idx, n, order):
    """the sum of v (values of the cells idx, ascending) in one of the three orders; cumsum is serial whatever the shape"""
    if not len(idx):
        return np.zeros(v.shape[1:])
    if order == "cell":
        return np.cumsum(v, axis=0)[-1]
    if order == "reverse":
        return np.cumsum(v[::-1], axis=0)[-1]
    parts = [np.cumsum(s, axis=0)[-1] for s in np.split(v, np.searchsorted(idx, np.arange(256, n, 256))) if len(s)]
    return np.cumsum(np.array(parts), axis=0)[-1]


def _cluster_sums(Xc, labels, k, order):
    n, d = Xc.shape
    sums, w = np.zeros((k, d)), np.zeros(k)
    for j in range(k):
        sel = np.flatnonzero(labels == j)
        w[j] = len(sel)
        sums[j] = _ordered_sum(Xc[sel], sel, n, order)
    return sums, w


def _sq4(a, b):
    """_euclidean_dense_dense(squared): four dimensions at a time, then the rest; rows of a against rows of b"""
    d = a.shape[-1]
    r = np.zeros(a.shape[:-1])
    t = 0
    while t + 4 <= d:
        q = (a[..., t:t + 4] - b[..., t:t + 4]) ** 2
        r = r + (((q[..., 0] + q[..., 1]) + q[..., 2]) + q[..., 3])
        t += 4
    while t < d:
        r = r + (a[..., t] - b[..., t]) ** 2
        t += 1
    return r


def _labels(Xc, centers, diag=None):
    dots = np.zeros((len(Xc), len(centers)))
    for t in range(Xc.shape[1]):
        dots += Xc[:, t][:, None] * centers[None, :, t]
    cc = np.zeros(len(centers))
    for t in range(Xc.shape[1]):
        cc += centers[:, t] * centers[:, t]
    v = cc[None, :] + -2.0 * dots
    if diag is not None and v.shape[1] > 1:
        s = np.sort(v, axis=1)
        # the gap between the two nearest centres relative to the squared distances themselves (||x||^2 added back)
        xx = (Xc * Xc).sum(axis=1)
        gap = (s[:, 1] - s[:, 0]) / np.maximum(np.abs(s[:, 1] + xx), 1e-300)
        dup = (centers[:, None, :] == centers[None, :, :]).all(axis=2)      # equal centres tie exactly in every arithmetic
        first, second = np.argsort(v, axis=1, kind="stable")[:, 0], np.argsort(v, axis=1, kind="stable")[:, 1]
        real = ~dup[first, second]
        if real.any():
            diag["gap"] = min(diag.get("gap", np.inf), float(gap[real].min()))
    return np.argmin(v, axis=1).astype(np.int32)


def lloyd(Xc, centers, tol, max_iter=300, order="cell", diag=None):
    """-> labels, centres (centred), n_iter, strict, relocations"""
    n, d = Xc.shape
    k = len(centers)
    centers = np.array(centers, dtype=np.float64)
    old = np.full(n, -1, np.int32)
    strict, relocs, n_iter = False, 0, max_iter
    for it in range(max_iter):
        labels = _labels(Xc, centers, diag)
        sums, w = _cluster_sums(Xc, labels, k, order)
        empty = np.flatnonzero(w == 0)
        if len(empty):
            dist = np.zeros(n)
            for t in range(d):
                dist += (Xc[:, t] - centers[labels, t]) ** 2
            if dist.max() != 0:
                far = np.lexsort((-np.arange(n), -dist))[:len(empty)]      # distance descending, then index descending
                for e, fi in zip(empty, far):
                    sums[labels[fi]] -= Xc[fi]
                    sums[e] = Xc[fi]
                    w[e] = 1.0
                    w[labels[fi]] -= 1.0
                    relocs += 1
        heavy = int(np.argmax(w))
        new = sums.copy()
        for j in range(k):      # in place and in order, so a weight-0 cluster below the heaviest one takes its RAW sum
            if w[j] > 0:
                new[j] *= 1.0 / w[j]
            else:
                new[j] = new[heavy]
        shift = np.sqrt(_sq4(new, centers))
        centers = new
        if np.array_equal(labels, old):
            strict, n_iter = True, it + 1
            break
        tot = float((shift ** 2).sum())
        if diag is not None and tol > 0:
            diag["tol"] = min(diag.get("tol", np.inf), abs(tot - tol) / tol)
        if tot <= tol:
            n_iter = it + 1
            break
        old = labels
    if not strict:
        labels = _labels(Xc, centers, diag)
    return labels, centers, n_iter, strict, relocs


# ---- steps 6, 7 ----------------------------------------------------------------------------------------------------------------------------
def db_sums(X, centers, labels, order="cell"):
    """per cluster the within sum of squares on the UNCENTRED matrix against the centres as returned, and the sizes"""
    k, d = centers.shape
    sq = np.zeros(len(X))
    for t in range(d):
        sq += (X[:, t] - centers[labels, t]) ** 2
    wss = np.zeros(k)
    for j in range(k):
        sel = np.flatnonzero(labels == j)
        wss[j] = _ordered_sum(sq[sel], sel, len(X), order)
    return wss, np.bincount(labels, minlength=k).astype(np.uint64)


def db_index(centers, wss, counts):
    k = len(centers)
    counts = np.where(np.asarray(counts) == 0, 1, counts).astype(np.float64)
    scatter = np.sqrt(np.asarray(wss, dtype=np.float64) / counts)
    dist = np.zeros((k, k))
    for i in range(k):
        for j in range(k):
            s = 0.0
            for t in range(centers.shape[1]):
                s += (centers[i, t] - centers[j, t]) ** 2
            dist[i, j] = math.sqrt(s)
    dist[np.abs(dist) < MIN_CENTROID_DIST] = MIN_CENTROID_DIST
    mix = (scatter + scatter[:, None]) / dist
    np.fill_diagonal(mix, 0.0)
    return float(np.max(mix, axis=1).sum() / k)


def relabel_by_size(labels, k):
    """labels 0-based -> clusters 1-based, the largest first, equal sizes in their own order"""
    sizes = np.bincount(np.asarray(labels) + 1, minlength=k + 1)
    order = np.argsort(np.argsort(-sizes, kind="stable"), kind="stable")
    return (1 + order[np.asarray(labels) + 1]).astype(np.int32)


# ---- the whole fit -------------------------------------------------------------------------------------------------------------------------
def fit(X, k, seed=0, init=None, max_iter=300, tol_factor=1e-4, order="cell", diag=None):
    X = np.ascontiguousarray(X, dtype=np.float64)
    Xc, mean, xx = center(X)
    tol = tolerance(X, tol_factor)
    seeds = None
    if init is None:
        u, first = seed_draws(seed, len(X), k)
        seeds = kmeans_plusplus(Xc, xx, k, u, first, diag)
        c0 = Xc[seeds]
    else:
        c0 = np.asarray(init, dtype=np.float64) - mean
    labels, cen, n_iter, strict, relocs = lloyd(Xc, c0, tol, max_iter, order, diag)
    inertia = _ordered_sum(_sq4(Xc, cen[labels]), np.arange(len(X)), len(X), order)
    centers = cen + mean
    wss, sizes = db_sums(X, centers, labels, order)
    return dict(labels=labels, centers=centers, inertia=float(inertia), n_iter=n_iter, strict=strict, relocations=relocs, seeds=seeds, wss=wss,
                sizes=sizes, db_score=db_index(centers, wss, sizes), clusters=relabel_by_size(labels, k), tol=tol)


# ---- fixtures ------------------------------------------------------------------------------------------------------------------------------
def blobs(n, d, n_blobs, seed):
    rs = np.random.RandomState(seed)
    c = rs.normal(0.0, 6.0, (n_blobs, d))
    return c[rs.randint(n_blobs, size=n)] + rs.normal(0.0, 1.0, (n, d))


# name -> dict(kind, n, d, ks, and for blobs: n_blobs; max_iter; the recorder adds the blob seed it settled on to the golden file)
FIXTURES = {
    "two_points": dict(kind="two_points", n=2, d=1, ks=[1, 2]),
    "n255": dict(kind="blobs", n=255, d=10, n_blobs=5, ks=[1, 2, 5, 10]),
    "n256": dict(kind="blobs", n=256, d=10, n_blobs=5, ks=[1, 2, 5, 10]),
    "n257": dict(kind="blobs", n=257, d=10, n_blobs=5, ks=[1, 2, 5, 10]),
    "one_dim": dict(kind="blobs", n=300, d=1, n_blobs=5, ks=[2, 5, 10]),
    "list_2_10": dict(kind="blobs", n=1000, d=10, n_blobs=6, ks=[2, 3, 4, 5, 6, 7, 8, 9, 10]),
    "n4099": dict(kind="blobs", n=4099, d=10, n_blobs=7, ks=[2, 5, 10]),
    "d50": dict(kind="blobs", n=5000, d=50, n_blobs=8, ks=[2, 5, 10]),
    "k64_d128": dict(kind="blobs", n=4099, d=128, n_blobs=40, ks=[64]),
    "n_equals_k": dict(kind="blobs", n=5, d=3, n_blobs=5, ks=[5]),
    "three_points": dict(kind="three_points", n=60, d=2, ks=[5]),
    "far_init": dict(kind="blobs", n=300, d=2, n_blobs=3, ks=[3], far_init=True),
    "round_limit": dict(kind="blobs", n=1000, d=10, n_blobs=6, ks=[10], max_iter=2),
    "equal_sizes": dict(kind="equal_sizes", n=200, d=2, ks=[2]),
}


def fixture_data(name, seed=0):
    """-> (X, init or None, max_iter)"""
    f = FIXTURES[name]
    init = None
    if f["kind"] == "two_points":
        X = np.array([[1.0], [4.0]])
    elif f["kind"] == "three_points":      # integers with an integer mean: every distance is exact and the potential ends at 0
        X = np.repeat(np.array([[0.0, 0.0], [6.0, 0.0], [0.0, 12.0]]), 20, axis=0)
    elif f["kind"] == "equal_sizes":
        rs = np.random.RandomState(1000 + seed)
        X = np.concatenate([rs.normal(-10.0, 1.0, (100, 2)), rs.normal(10.0, 1.0, (100, 2))])
    else:
        X = blobs(f["n"], f["d"], f["n_blobs"], 100 + seed)
    if f.get("far_init"):      # two centres inside the data, the third so far away that no point is nearest to it
        init = np.array([X[0], X[1], X.max(axis=0) + 1000.0])
    return np.ascontiguousarray(X), init, f.get("max_iter", 300)
