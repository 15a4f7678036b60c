"""RUN_TSNE restated in numpy, in the sum orders include/crgpu.h states for csrc/tsne.hip (no GPU).

The stage calls a port of van der Maaten's bh_tsne whose source the reference does not carry; this file is the published algorithm in
its theta = 0 limit, and the library is checked against it.  np.cumsum along an axis adds left to right in f64, which is how every
ordered sum below is written; a trailing +0.0 moves no bit of such a sum, so ragged rows are padded with zeros.

The descent (gradient, update, centring) holds + - * / only: given the same P and Y the device's trajectory equals this one bit for
bit.  exp (the search) and log (the cost) are libm's here and OCML's there.
"""
import collections
import sys

import numpy as np

import knn_numpy

CAND_CHUNK = 4096      # CRGPU_TSNE_CAND_CHUNK
PART_ROWS = 256        # rows of a partial of the column sums
MAX_STEPS = 200
TOL = 1e-5
DBL_MIN, DBL_MAX = sys.float_info.min, sys.float_info.max
FLT_MIN = float(np.finfo(np.float32).tiny)
EXAGGERATION, ETA = 12.0, 200.0


def ordered_sum(a):
    """The column sums of a [n] or [n, c] over partials of 256 rows, left to right within one, then the partials ascending"""
    a = np.asarray(a, dtype=np.float64)
    flat = a.ndim == 1
    a = a.reshape(len(a), -1)
    pad = (-len(a)) % PART_ROWS
    a = np.concatenate([a, np.zeros((pad, a.shape[1]))]) if pad else a
    parts = np.cumsum(a.reshape(-1, PART_ROWS, a.shape[1]), axis=1)[:, -1, :]
    out = np.cumsum(parts, axis=0)[-1]
    return float(out[0]) if flat else out


def stage_perplexity(n, perplexity):
    """bhtsne.py:57-64 -> (the perplexity used, True when the projection is defined as all zeros)"""
    perplexity = min(perplexity, max(1, -1 + float(n - 1) / 3))
    return perplexity, n - 1 < 3 * perplexity


def normalize(x):
    x = np.array(x, dtype=np.float64)
    x -= np.cumsum(x, axis=0)[-1] / x.shape[0]
    top = np.abs(x).max()
    return x / top if top > 0 else x


def search(dist, perplexity):
    """The bisection on beta of every row of dist f64[n, k] (distances, by rank)
    -> dict(beta, steps, cond [n, k], lo, hi: the bounds a row ended with, hdiff: every H - log(perplexity) that decided a step)"""
    dist = np.asarray(dist, dtype=np.float64)
    n, k = dist.shape
    d2 = dist * dist
    logp = np.log(perplexity)
    beta, lo, hi = np.ones(n), np.full(n, -DBL_MAX), np.full(n, DBL_MAX)
    used, s_used, steps = np.ones(n), np.full(n, DBL_MIN), np.zeros(n, np.uint32)
    active = np.ones(n, bool)
    hdiff = []
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        for _ in range(MAX_STEPS):
            r = np.flatnonzero(active)
            if not len(r):
                break
            bd = beta[r, None] * d2[r]
            p = np.exp(-bd)
            s = DBL_MIN + np.cumsum(p, axis=1)[:, -1]
            H = np.cumsum(bd * p, axis=1)[:, -1] / s + np.log(s)
            diff = H - logp
            hdiff.append(diff)
            used[r], s_used[r] = beta[r], s
            steps[r] += 1
            found = np.abs(diff) < TOL
            up, down = r[~found & (diff > 0)], r[~found & ~(diff > 0)]
            lo[up] = beta[up]
            fresh = (hi[up] == DBL_MAX) | (hi[up] == -DBL_MAX)
            beta[up] = np.where(fresh, beta[up] * 2.0, (beta[up] + hi[up]) / 2.0)
            hi[down] = beta[down]
            fresh = (lo[down] == -DBL_MAX) | (lo[down] == DBL_MAX)
            beta[down] = np.where(fresh, beta[down] / 2.0, (beta[down] + lo[down]) / 2.0)
            active[r[found]] = False
        cond = np.exp(-(used[:, None] * d2)) / s_used[:, None]
    return dict(beta=used, steps=steps, cond=cond, lo=lo, hi=hi, hdiff=np.concatenate(hdiff), d2=d2, s=s_used)


def symmetrize(ind, cond):
    """-> (indptr i64[n + 1], indices i32[nnz], values before the normalisation, the total, values) of the union of both directions"""
    ind = np.asarray(ind, dtype=np.int64)
    n, k = ind.shape
    rows = np.repeat(np.arange(n, dtype=np.int64), k)
    cols = ind.reshape(-1)
    keys = np.concatenate([rows * n + cols, cols * n + rows])
    p = np.concatenate([cond.reshape(-1), cond.reshape(-1)])
    uniq, inv = np.unique(keys, return_inverse=True)
    merged = np.bincount(inv, weights=p, minlength=len(uniq)) / 2.0      # one or two members of a key: a + b = b + a
    indptr = np.searchsorted(uniq, np.arange(n + 1, dtype=np.int64) * n).astype(np.int64)
    total = ordered_sum(merged)
    return indptr, (uniq % n).astype(np.int32), merged, total, merged / total


def affinities(ind, dist, perplexity):
    s = search(dist, perplexity)
    indptr, indices, merged, total, values = symmetrize(ind, s["cond"])
    s.update(indptr=indptr, indices=indices, merged=merged, p_total=total, values=values)
    return s


def _rows_left_to_right(indptr, terms):
    """terms f64[nnz, c] -> f64[n, c]: a row's entries added left to right from 0.0"""
    n, lens = len(indptr) - 1, np.diff(indptr)
    width = max(1, int(lens.max()))
    dense = np.zeros((n, width, terms.shape[1]))
    rows = np.repeat(np.arange(n), lens)
    pos = np.arange(len(terms)) - np.repeat(indptr[:-1], lens)
    dense[rows, pos] = terms
    return np.cumsum(dense, axis=1)[:, -1, :]


def repulsion(Y, chunk=CAND_CHUNK):
    """-> (z f64[n], neg f64[n, dims]): the candidates in chunks, left to right within one, a row's chunk partials left to right"""
    n, dims = Y.shape
    z, neg = np.zeros(n), np.zeros((n, dims))
    for r0 in range(0, n, 1024):      # rows are independent: blocks of them only bound the memory
        r1 = min(n, r0 + 1024)
        for c0 in range(0, n, chunk):
            c1 = min(n, c0 + chunk)
            v = [Y[r0:r1, None, t] - Y[None, c0:c1, t] for t in range(dims)]
            d2 = np.zeros((r1 - r0, c1 - c0))
            for t in range(dims):
                d2 = d2 + v[t] * v[t]
            q = 1.0 / (1.0 + d2)
            same = np.arange(max(r0, c0), min(r1, c1))
            q[same - r0, same - c0] = 0.0      # the pair (i, i) is no pair
            z[r0:r1] = z[r0:r1] + np.cumsum(q, axis=1)[:, -1]
            qq = q * q
            for t in range(dims):
                neg[r0:r1, t] = neg[r0:r1, t] + np.cumsum(qq * v[t], axis=1)[:, -1]
    return z, neg


def _entry_terms(indptr, indices, Y):
    rows = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))
    v = Y[rows] - Y[indices]
    d2 = np.zeros(len(rows))
    for t in range(Y.shape[1]):
        d2 = d2 + v[:, t] * v[:, t]
    return v, 1.0 / (1.0 + d2)


def gradient(indptr, indices, values, Y, exaggeration=1.0, chunk=CAND_CHUNK):
    """-> (dC f64[n, dims] = bh_tsne's gradient, a quarter of the analytic one; Z)"""
    z, neg = repulsion(Y, chunk)
    Z = ordered_sum(z)
    v, q = _entry_terms(indptr, indices, Y)
    pos = _rows_left_to_right(indptr, ((exaggeration * values) * q)[:, None] * v)
    return pos - neg / Z, Z


def cost(indptr, indices, values, Y, Z=None):
    if Z is None:
        Z = ordered_sum(repulsion(Y)[0])
    _, q = _entry_terms(indptr, indices, Y)
    terms = values * np.log((values + FLT_MIN) / (q / Z + FLT_MIN))
    return ordered_sum(_rows_left_to_right(indptr, terms[:, None])[:, 0])


def step(indptr, indices, values, Y, uY, gains, it, stop_lying_iter, mom_switch_iter, eta=ETA):
    """One iteration -> (Y, uY, gains)"""
    dC, _ = gradient(indptr, indices, values, Y, EXAGGERATION if it < stop_lying_iter else 1.0)
    gains = np.where(np.sign(dC) != np.sign(uY), gains + 0.2, gains * 0.8)
    gains = np.where(gains < 0.01, 0.01, gains)
    uY = ((0.5 if it < mom_switch_iter else 0.8) * uY) - ((eta * gains) * dC)
    Y = Y + uY
    return Y - ordered_sum(Y) / float(len(Y)), uY, gains


def run(indptr, indices, values, Y, first_iter, n_iters, stop_lying_iter, mom_switch_iter, uY=None, gains=None, keep=()):
    """The iterations first_iter .. first_iter + n_iters -> (Y, uY, gains, {k: (Y, uY, gains) after k iterations in all, k in keep})"""
    Y = np.array(Y, dtype=np.float64)
    uY = np.zeros_like(Y) if uY is None else np.array(uY)
    gains = np.ones_like(Y) if gains is None else np.array(gains)
    kept = {}
    for it in range(first_iter, first_iter + n_iters):
        Y, uY, gains = step(indptr, indices, values, Y, uY, gains, it, stop_lying_iter, mom_switch_iter)
        if it + 1 in keep:
            kept[it + 1] = (Y.copy(), uY.copy(), gains.copy())
    return Y, uY, gains, kept


def start(seed, n, dims):
    """np.random.RandomState(seed).randn(n * dims) * 1e-4, row-major: what crgpu_legacy_randn restates"""
    return (np.random.RandomState(seed).randn(n * dims) * 1e-4).reshape(n, dims)


# ---- fixtures ----------------------------------------------------------------------------------------------------------------------------
def _three_groups():
    rs = np.random.RandomState(20261021)
    centres = rs.normal(size=(3, 10)) * 20.0
    return np.concatenate([centres[g] + rs.normal(size=(100, 10)) for g in range(3)])


def _two_groups_130():
    rs = np.random.RandomState(20261022)
    centres = rs.normal(size=(2, 5)) * 8.0
    return np.concatenate([centres[g] + rs.normal(size=(65, 5)) for g in range(2)])


def _duplicates():
    x = np.random.RandomState(20261023).normal(size=(120, 4))
    x[1:17] = x[0]      # K + 2 = 17 equal rows at K = 15: each keeps itself or a twin at distance 0, all K distances 0
    return x


def _hub():
    x = np.random.RandomState(20261024).normal(size=(130, 60))
    x[57] = 0.0         # in 60 dimensions the origin is nearer to every row than any other row is: every row names row 57
    return x


def _chain():
    # row i at 4^-i on a line: the three nearest rows of i are i + 1, i + 2, i + 3, none of which names i back (the closest rows
    # of a finite set are always mutual, so the last rows of the chain name each other: one direction only everywhere else).
    # Every row's search samples one function at powers of two, so the maker accepts or rejects them together: the ratio 1 / 2
    # is rejected (a step lands within 1e-9 of 0), 1 / 4 is not
    return (0.25 ** np.arange(24.0))[:, None]


Fixture = collections.namedtuple("Fixture", "x perplexity dims seed")
FIXTURES = collections.OrderedDict([
    ("three_groups", Fixture(_three_groups(), 30, 2, 0)),
    ("two_groups_130", Fixture(_two_groups_130(), 10, 2, 3)),
    ("duplicates", Fixture(_duplicates(), 5, 2, 1)),
    ("hub", Fixture(_hub(), 5, 3, 2)),
    ("chain", Fixture(_chain(), 1, 2, 4)),
])
# K = 1024, the limit: too large for the golden file, the device is held to the restatement alone (same rejection rule)
NOT_IN_GOLDEN = collections.OrderedDict([
    ("k1024", Fixture(np.random.RandomState(20261027).normal(size=(1100, 2)), 341.5, 2, 5)),
])
ALL_ZERO = Fixture(np.random.RandomState(20261025).normal(size=(3, 4)), 30, 2, 0)   # N - 1 = 2 < 3 * 1
SKLEARN_FIXTURES = ("three_groups", "two_groups_130", "hub")      # no entry (i, i): P has a condensed form
TRAJECTORY = dict(name="two_groups_130", max_iter=300, stop_lying_iter=100, mom_switch_iter=120, keep=(1, 99, 100, 101, 120, 121, 300))

_cache = {}


def synthetic_problem(n, dims, seed, decades=0.0):
    """A CSR P and a Y for the gradient at a constructed size: row i names i + 1, i + 5 and the hub 0 (the hub names 1, 2, 3), so
    row 0 holds n - 1 entries beside rows of about 5; rows 3 and 4 of Y coincide (q = 1); decades > 0 spreads |Y| over that many
    -> (indptr, indices, values, Y)"""
    rs = np.random.RandomState(seed)
    i = np.arange(n)
    ind = np.stack([(i + 1) % n, (i + 5) % n, np.zeros(n, np.int64)], axis=1)
    ind[0] = [1, 2, 3]
    indptr, indices, _, _, values = symmetrize(ind, rs.uniform(0.01, 1.0, size=(n, 3)))
    Y = rs.normal(size=(n, dims)) * 3.0
    if decades:
        Y *= 10.0 ** rs.uniform(-decades / 2, decades / 2, size=(n, 1))
    Y[4] = Y[3]
    return indptr, indices, values, Y


def prepared(name):
    """A fixture's normalised input, neighbours and affinities, computed once and shared; treat as read-only"""
    if name not in _cache:
        f = FIXTURES[name] if name in FIXTURES else NOT_IN_GOLDEN[name]
        perplexity, zero = stage_perplexity(len(f.x), f.perplexity)
        assert not zero
        x = normalize(f.x)
        k = int(3 * perplexity)
        ind, dist, _ = knn_numpy.knn(x, k)
        a = affinities(ind, dist, perplexity)
        a.update(x=x, k=k, perplexity=perplexity, nn_indices=ind, nn_distances=dist, y0=start(f.seed, len(x), f.dims))
        _cache[name] = a
    return _cache[name]
