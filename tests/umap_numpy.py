"""RUN_UMAP restated in numpy, in the sum orders include/crgpu.h states for csrc/umap.hip (no GPU).

The stage calls the crate umap-rs, whose source the reference does not carry; this file is the published algorithm (McInnes et al., as
umap-learn states it) with the layout in the per-epoch batch form, and the library is checked against it.  np.cumsum along an axis adds
left to right in f64, which is how every ordered sum below is written; a trailing +0.0 moves no bit of such a sum, so ragged rows are
padded with zeros.

The schedule, the sampled vertices and the branches hold + - * /, floor and integers only: given the same graph and Y the device's
equal these bit for bit.  exp (the search, the memberships) and pow (the terms) are libm's here and OCML's there.
"""
import collections

import numpy as np

import knn_numpy

PART_ROWS = 256        # rows of a partial of the distance total
MAX_STEPS = 64
TOL = 1e-5
FLOOR = 1e-3           # umap-learn's MIN_K_DIST_SCALE
SLOTS = 16             # CRGPU_UMAP_SLOTS: Philox words of an entry per epoch
MAX_NEG = 15           # n_neg <= 2 rate - 1 at the largest rate, 8
N_NEIGHBORS, MIN_DIST, SPREAD, RATE = 30, 0.3, 1.0, 5
METRICS = ("correlation", "pearson", "cosine", "euclidean")


def ordered_sum(a):
    """The sum of a [n] over partials of 256 rows, left to right within one, then the partials ascending"""
    a = np.asarray(a, dtype=np.float64)
    pad = (-len(a)) % PART_ROWS
    a = np.concatenate([a, np.zeros(pad)]) if pad else a
    return float(np.cumsum(np.cumsum(a.reshape(-1, PART_ROWS), axis=1)[:, -1])[-1])


def stage_neighbors(n, n_neighbors=N_NEIGHBORS):
    """umap.rs -> (n_neighbors used, True when the projection is defined as all zeros)"""
    return min(n_neighbors, n - 1), n < 3


def default_epochs(n):
    return 500 if n <= 10000 else 200


def metric_input(x, metric="correlation"):
    """-> (the rows the neighbour search runs on, True when the dissimilarity is 0.5 * (dist * dist))"""
    assert metric in METRICS
    x = np.array(x, dtype=np.float64)
    if metric == "euclidean":
        return x, False
    if metric != "cosine":
        x -= (np.cumsum(x, axis=1)[:, -1] / x.shape[1])[:, None]
    norm = np.sqrt(np.cumsum(x * x, axis=1)[:, -1])
    return x / np.where(norm > 0, norm, 1.0)[:, None], True


def rescale(y):
    y = np.array(y, dtype=np.float64)
    lo, hi = y.min(axis=0), y.max(axis=0)
    span = hi - lo
    return np.where(span > 0, 10.0 * (y - lo) / np.where(span > 0, span, 1.0), 0.0)


# ---- the curve ---------------------------------------------------------------------------------------------------------------------------
def curve(min_dist, spread):
    x = np.linspace(0, 3 * spread, 300)
    return x, np.where(x < min_dist, 1.0, np.exp(-(x - min_dist) / spread))


def umap_ab(min_dist=MIN_DIST, spread=SPREAD):
    """Levenberg-Marquardt from (1, 1) on the 300 points, the 2 x 2 normal equations solved directly; a step is taken when the cost
    does not rise by more than its own rounding; it ends when a taken step is below 1e-12 of the parameters -> (a, b)"""
    x, y = curve(min_dist, spread)
    lx = np.log(np.where(x > 0, x, 1.0))

    def cost_of(a, b):
        r = 1.0 / (1.0 + a * np.power(x, 2.0 * b)) - y
        return float(np.cumsum(r * r)[-1])

    a, b, lam = 1.0, 1.0, 1e-3
    cost = cost_of(a, b)
    for _ in range(500):
        p = np.power(x, 2.0 * b)
        f = 1.0 / (1.0 + a * p)
        r = f - y
        ja, jb = -(p * (f * f)), np.where(x > 0, -((a * p) * (2.0 * lx) * (f * f)), 0.0)
        A00, A01, A11, g0, g1 = (float(np.cumsum(v)[-1]) for v in (ja * ja, ja * jb, jb * jb, ja * r, jb * r))
        taken = False
        for _ in range(60):
            B00, B11 = A00 + lam * A00, A11 + lam * A11
            det = B00 * B11 - A01 * A01
            if det > 0:
                da, db = (-g0 * B11 + g1 * A01) / det, (-g1 * B00 + g0 * A01) / det
                if np.isfinite(da) and np.isfinite(db) and a + da > 0 and b + db > 0:
                    cn = cost_of(a + da, b + db)
                    taken = cn <= cost + 1e-14 * cost
            lam = max(lam / 10.0, 1e-15) if taken else lam * 10.0
            if taken:
                break
        if not taken:
            break
        rel = np.sqrt(da * da + db * db) / np.sqrt(a * a + b * b)
        a, b, cost = a + da, b + db, cn
        if rel < 1e-12:
            break
    return a, b


# ---- the fuzzy graph ---------------------------------------------------------------------------------------------------------------------
def search(dist):
    """rho, the search for sigma and the memberships of every row of dist f64[n, k] (dissimilarities, by rank)
    -> dict(rho, mid, sigma, steps, memb [n, k], floored, decisions: every psum - log2(k + 1) that decided a step)"""
    dist = np.asarray(dist, dtype=np.float64)
    n, k = dist.shape
    positive = dist > 0
    rho = np.where(positive.any(axis=1), dist[np.arange(n), np.argmax(positive, axis=1)], 0.0)
    rowsum = np.cumsum(dist, axis=1)[:, -1]
    total = ordered_sum(rowsum)
    target = float(np.log2(k + 1))
    lo, hi, mid = np.zeros(n), np.full(n, np.inf), np.ones(n)
    steps, active, decisions = np.zeros(n, np.uint32), np.ones(n, bool), []
    x = dist - rho[:, None]
    with np.errstate(over="ignore", under="ignore", invalid="ignore", divide="ignore"):
        for _ in range(MAX_STEPS):
            r = np.flatnonzero(active)
            if not len(r):
                break
            psum = np.cumsum(np.where(x[r] > 0, np.exp(-(x[r] / mid[r, None])), 1.0), axis=1)[:, -1]
            steps[r] += 1
            decisions.append(psum - target)
            found = np.abs(psum - target) < TOL
            up, down = r[~found & (psum > target)], r[~found & ~(psum > target)]
            hi[up] = mid[up]
            mid[up] = (lo[up] + hi[up]) / 2.0
            lo[down] = mid[down]
            mid[down] = np.where(np.isinf(hi[down]), mid[down] * 2.0, (lo[down] + hi[down]) / 2.0)
            active[r[found]] = False
        m = np.where(rho > 0, rowsum / float(k + 1), total / (float(n) * float(k + 1)))
        sigma = np.where(mid < FLOOR * m, FLOOR * m, mid)
        memb = np.where((x <= 0) | (sigma[:, None] == 0), 1.0, np.exp(-(x / sigma[:, None])))
    return dict(rho=rho, mid=mid, sigma=sigma, steps=steps, memb=memb, floored=mid < FLOOR * m, decisions=np.concatenate(decisions), x=x, target=target)


def union(ind, memb):
    """-> (keys i * n + j ascending, a, b: the memberships of the one or two members of a key (b 0 when alone), (a + b) - a * b)"""
    ind = np.asarray(ind, dtype=np.int64)
    n, k = ind.shape
    rows, cols = np.repeat(np.arange(n, dtype=np.int64), k), ind.reshape(-1)
    keys = np.concatenate([rows * n + cols, cols * n + rows])
    w = np.concatenate([memb.reshape(-1), memb.reshape(-1)])
    order = np.argsort(keys, kind="stable")
    uniq, first, count = np.unique(keys[order], return_index=True, return_counts=True)
    assert count.max() <= 2
    a = w[order[first]]
    b = np.where(count == 2, w[order[np.minimum(first + 1, len(order) - 1)]], 0.0)
    return uniq, a, b, (a + b) - a * b


def graph(ind, dist, n_epochs):
    """-> dict(rho, sigma, steps, memb, indptr i64[n + 1], indices i32[nnz], values f64[nnz], wmax, the union before the prune)"""
    g = search(dist)
    n = len(dist)
    keys, a, b, merged = union(ind, g["memb"])
    wmax = float(merged.max())
    keep = merged >= wmax / float(n_epochs)
    kept = keys[keep]
    g.update(indptr=np.searchsorted(kept, np.arange(n + 1, dtype=np.int64) * n).astype(np.int64), indices=(kept % n).astype(np.int32),
             values=merged[keep], wmax=wmax, nnz=int(keep.sum()), union_keys=keys, union_a=a, union_b=b, union_values=merged, keep=keep,
             threshold=wmax / float(n_epochs))
    return g


# ---- the epochs --------------------------------------------------------------------------------------------------------------------------
def philox_words(seed, epoch, count):
    """The first `count` words of Philox stream `epoch` with key seed, in csrc/philox.h's numbering"""
    return np.random.Philox(counter=[0, int(epoch), 0, 0], key=[int(seed), 0]).random_raw(int(count)) if count else np.zeros(0, np.uint64)


def _rows_left_to_right(n, row_of, terms):
    """terms f64[m, c] of the rows row_of (ascending) -> f64[n, c]: a row's terms added left to right from 0.0"""
    out = np.zeros((n, terms.shape[1]))
    if not len(terms):
        return out
    lens = np.bincount(row_of, minlength=n)
    start = np.cumsum(lens) - lens
    dense = np.zeros((n, int(lens.max()), terms.shape[1]))
    dense[row_of, np.arange(len(terms)) - start[row_of]] = terms
    return np.cumsum(dense, axis=1)[:, -1, :]


def clip(x):
    return np.where(x > 4.0, 4.0, np.where(x < -4.0, -4.0, x))


def terms(Y, i, other, attract, a, b, gamma=1.0):
    """The terms of the rows i against the vertices `other` -> (term f64[m, dims], d2, c * v before the clip)"""
    v = Y[i] - Y[other]
    d2 = np.zeros(len(v))
    for t in range(Y.shape[1]):
        d2 = d2 + v[:, t] * v[:, t]
    pos = d2 > 0
    safe = np.where(pos, d2, 1.0)
    p = np.power(safe, b)
    den = a * p + 1.0
    if attract:
        c = np.where(pos, (((-2.0 * a) * b) * (p / safe)) / den, 0.0)
    else:
        c = np.where(pos, ((2.0 * gamma) * b) / ((0.001 + safe) * den), 0.0)
    raw = c[:, None] * v
    x = clip(raw)
    return (2.0 * x if attract else x), d2, raw


def schedule(values, wmax, rate=RATE):
    """-> (eps, epns): the two states start at them"""
    eps = wmax / values
    return eps, eps / float(rate)


def epoch(indptr, indices, values, Y, eons, eonns, n, n_epochs, a, b, seed, gamma=1.0, initial_alpha=1.0, rate=RATE, wmax=None, detail=False):
    """Epoch n -> (Y', eons', eonns', info: active entries, n_neg of each, the sampled vertices, delta, sum |terms| and the term count
    per row).  Every term is taken from Y as given"""
    N, nnz = len(indptr) - 1, len(values)
    wmax = float(values.max()) if wmax is None else wmax
    eps, epns = schedule(values, wmax, rate)
    nd = float(n)
    alpha = initial_alpha * (1.0 - nd / float(n_epochs))
    row_of_entry = np.repeat(np.arange(N), np.diff(indptr))
    act = np.flatnonzero(eons <= nd)
    n_neg = np.floor((nd - eonns[act]) / epns[act]).astype(np.int64)
    assert (n_neg >= 0).all() and (n_neg <= MAX_NEG).all() and MAX_NEG < SLOTS, "n_neg = %s" % n_neg.max()
    words = philox_words(seed, n, nnz * SLOTS)
    which = np.repeat(np.arange(len(act)), n_neg)
    s = np.arange(len(which)) - np.repeat(np.cumsum(n_neg) - n_neg, n_neg)
    e_neg = act[which]
    kk = (words[e_neg * SLOTS + s] % np.uint64(N)).astype(np.int64)
    t_att, d2_att, raw_att = terms(Y, row_of_entry[act], indices[act], True, a, b, gamma)
    t_neg, d2_neg, raw_neg = terms(Y, row_of_entry[e_neg], kk, False, a, b, gamma)
    t_neg[kk == row_of_entry[e_neg]] = 0.0      # the row itself contributes nothing
    entry, slot = np.concatenate([act, e_neg]), np.concatenate([np.zeros(len(act), np.int64), 1 + s])
    order = np.lexsort((slot, entry))           # (entry, attraction, then s ascending)
    all_terms, row_of = np.concatenate([t_att, t_neg])[order], row_of_entry[entry[order]]
    delta = _rows_left_to_right(N, row_of, all_terms)
    eons2, eonns2 = eons.copy(), eonns.copy()
    eons2[act] = eons[act] + eps[act]
    eonns2[act] = eonns[act] + n_neg.astype(np.float64) * epns[act]
    Ynew = Y + alpha * delta
    info = dict(active=act, n_neg=n_neg, kk=kk, delta=delta, alpha=alpha, n_active=len(act), n_negative=int(n_neg.sum()))
    if detail:
        info.update(sum_abs=_rows_left_to_right(N, row_of, np.abs(all_terms)), n_terms=np.bincount(row_of, minlength=N), d2_att=d2_att, d2_neg=d2_neg,
                    raw_att=raw_att, raw_neg=raw_neg, self_sample=kk == row_of_entry[e_neg], e_neg=e_neg, s=s)
    return Ynew, eons2, eonns2, info


def run(indptr, indices, values, Y, first_epoch, n_run, n_epochs, a, b, seed, eons=None, eonns=None, rate=RATE, keep=()):
    """The epochs first_epoch .. first_epoch + n_run -> (Y, eons, eonns, totals, {k: (Y, eons, eonns) after k epochs in all, k in keep})"""
    Y = np.array(Y, dtype=np.float64)
    wmax = float(values.max())
    if first_epoch == 0:
        eons, eonns = schedule(values, wmax, rate)
    kept, totals = {}, dict(n_active=0, n_negative=0, largest_move=0.0, max_n_neg=0)
    for n in range(first_epoch, first_epoch + n_run):
        Ynew, eons, eonns, info = epoch(indptr, indices, values, Y, eons, eonns, n, n_epochs, a, b, seed, rate=rate, wmax=wmax)
        totals["n_active"] += info["n_active"]
        totals["n_negative"] += info["n_negative"]
        totals["largest_move"] = max(totals["largest_move"], float(np.abs(Ynew - Y).max()))
        totals["max_n_neg"] = max(totals["max_n_neg"], int(info["n_neg"].max()) if len(info["n_neg"]) else 0)
        Y = Ynew
        if n + 1 in keep:
            kept[n + 1] = (Y.copy(), eons.copy(), eonns.copy())
    return Y, eons, eonns, totals, kept


# ---- fixtures ----------------------------------------------------------------------------------------------------------------------------
def _three_groups(size=100):
    rs = np.random.RandomState(20261101)
    centres = rs.normal(size=(3, 10)) * 20.0
    return np.concatenate([centres[g] + rs.normal(size=(size, 10)) for g in range(3)])


def _duplicates():
    x = np.random.RandomState(20261102).normal(size=(120, 4))
    x[1:17] = x[0]      # k + 2 = 17 equal rows at k = 15: all k distances 0, rho = 0, the all-distances floor, the entry (i, i)
    return x


def _hub():
    x = np.random.RandomState(20261103).normal(size=(130, 60))
    x[57] = 0.0         # in 60 dimensions the origin is nearer to every row than any other row is: every row names row 57
    return x


def _chain():
    # row i at 4^-i on a line: the nearest row of i is i + 1, which does not name i back (but for the last two rows)
    return (0.25 ** np.arange(24.0))[:, None]


def _zero_variance():
    x = np.random.RandomState(20261104).normal(size=(40, 6)) + np.arange(6.0)
    x[7] = 3.25         # a constant row: the zero vector under correlation
    return x


Fixture = collections.namedtuple("Fixture", "x n_neighbors metric dims seed n_epochs")
FIXTURES = collections.OrderedDict([
    ("three_groups", Fixture(_three_groups(), 30, "correlation", 2, 0, 500)),
    ("duplicates", Fixture(_duplicates(), 16, "euclidean", 2, 1, 200)),
    ("hub", Fixture(_hub(), 6, "euclidean", 3, 2, 200)),
    ("chain", Fixture(_chain(), 2, "euclidean", 2, 4, 120)),
    ("zero_variance", Fixture(_zero_variance(), 8, "correlation", 2, 3, 200)),
])
TWO_ROWS = Fixture(np.random.RandomState(20261105).normal(size=(2, 4)), 30, "correlation", 2, 0, 500)      # N = 2: all zeros
AB_CASES = ((0.3, 1.0), (0.1, 1.0), (0.001, 1.0), (0.5, 2.0))

_cache = {}


def start(f):
    """The start of a fixture: the first dims columns of its input, or (fewer columns than dimensions) seeded normal rows; rescaled"""
    y = f.x[:, :f.dims] if f.x.shape[1] >= f.dims else np.random.RandomState(f.seed).normal(size=(len(f.x), f.dims))
    return rescale(y)


def prepared(name):
    """A fixture's prepared rows, neighbours, graph and start, computed once and shared; treat as read-only"""
    if name not in _cache:
        f = FIXTURES[name]
        n_neighbors, zero = stage_neighbors(len(f.x), f.n_neighbors)
        assert not zero
        rows, angular = metric_input(f.x, f.metric)
        k = n_neighbors - 1
        ind, dist, _ = knn_numpy.knn(rows, k)
        d = 0.5 * (dist * dist) if angular else dist
        g = graph(ind, d, f.n_epochs)
        g.update(rows=rows, k=k, nn_indices=ind, nn_distances=d, y0=start(f), n_epochs=f.n_epochs, seed=f.seed, dims=f.dims)
        _cache[name] = g
    return _cache[name]


def synthetic_graph(n, dims, seed, hub=True):
    """A symmetric CSR graph and a Y at a constructed size: row i names i + 1 and i + 5, and every row names the hub 0 (which names 1,
    2, 3), so row 0 holds n - 1 entries beside rows of 4 and 5; the weights are drawn so that an entry's twin carries the same bits;
    rows 3 and 4 of Y coincide (d2 = 0) -> (indptr, indices, values, Y)"""
    rs = np.random.RandomState(seed)
    i = np.arange(n)
    ind = np.stack([(i + 1) % n, (i + 5) % n, np.zeros(n, np.int64) if hub else (i + 9) % n], axis=1)
    if hub:
        ind[0] = [1, 2, 3]
    memb = rs.uniform(0.05, 1.0, size=(n, 3))
    memb[:, 0] = 1.0      # the nearest neighbour: wmax = 1
    keys, _, _, values = union(ind, memb)
    indptr = np.searchsorted(keys, np.arange(n + 1, dtype=np.int64) * n).astype(np.int64)
    Y = rs.uniform(0.0, 10.0, size=(n, dims))
    Y[4] = Y[3]
    return indptr, (keys % n).astype(np.int32), values, Y
