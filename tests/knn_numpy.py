"""The exact k-nearest-neighbour query of RUN_GRAPH_CLUSTERING restated in numpy, and the fixtures of its tests.

compute_nearest_neighbors (analysis/graphclust.py:39-62) is BallTree(x, leaf_size).query(rows, k + 1) of scikit-learn 1.7.2 followed by
[:, 1:].  The tree only prunes; what comes out is brute force:
  * d2(i, j) = the sum over t = 0 .. d - 1 of (x_it - x_jt) * (x_it - x_jt), added in dimension order, f64, no fused multiply-add
    (numpy's elementwise multiply and add are two roundings);
  * the pairs (d2, j) over ALL rows j, i included, in ascending order, the lower index first among equal d2;
  * the first pair is dropped -- the row itself unless an exact duplicate of lower index exists, which is then dropped in its place;
  * the distance is np.sqrt(d2).
On tie-free input BallTree gives these indices; on tied input it gives these distances, and its indices follow its own traversal.

FIXTURES: name -> dict(x f64[n, columns], k, num_pcs (None = all columns), tied).  Generated from the RandomState seeds below; small.
tests/golden/knn_reference.npz (scripts/make_knn_golden.py) holds BallTree's answer for a seeded sample of the rows of each.
"""
import collections

import numpy as np

QUERY_TILE = 64        # queries of a workgroup (csrc/knn.hip): what `compactions` is counted per


def d2_rows(x, lo, hi):
    """f64[hi - lo, n]: the squared distances of the rows lo .. hi to every row, in dimension order, unfused"""
    x = np.asarray(x, dtype=np.float64)
    acc = np.zeros((hi - lo, x.shape[0]))
    for t in range(x.shape[1]):
        diff = x[lo:hi, t][:, None] - x[None, :, t]
        acc += diff * diff
    return acc


def knn(x, k, query_start=0, n_queries=None, chunk=512):
    """-> (indices i32[q, k], distances f64[q, k], d2 f64[q, k]) of the rows query_start .. query_start + n_queries"""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    q1 = n if n_queries is None else query_start + n_queries
    ind, d2 = [], []
    for lo in range(query_start, q1, chunk):
        hi = min(lo + chunk, q1)
        a = d2_rows(x, lo, hi)
        order = np.argsort(a, axis=1, kind="stable")[:, 1:k + 1]      # stable: the lower index first among equal d2
        ind.append(order.astype(np.int32))
        d2.append(np.take_along_axis(a, order, axis=1))
    ind, d2 = np.concatenate(ind), np.concatenate(d2)
    return ind, np.sqrt(d2), d2


def is_pair_order(x, row, indices, k):
    """True when `indices` are the k entries after the first of row's pairs in (d2, index) order -- checked without a sort"""
    a = d2_rows(x, row, row + 1)[0]
    keys = list(zip(a.tolist(), range(len(a))))
    chosen = [keys[j] for j in indices]
    if chosen != sorted(chosen) or len(set(indices.tolist())) != k:
        return False
    first = min(keys)
    rest = sorted(set(keys) - {first})[:k]
    return rest == chosen


def num_neighbors(n, given=1, a=-230.0, b=120.0):
    """split()'s rule, restated"""
    use = int(max(given, np.round(a + b * np.log10(n))))
    return max(1, min(use, n - 1))


def _normal(seed, n, d):
    return np.random.RandomState(seed).normal(size=(n, d))


def _clustered(seed):
    rs = np.random.RandomState(seed)
    sizes = [1000, 800, 600, 400, 200]                                # each above k + 1: no neighbour outside the own cluster
    centres = rs.normal(size=(5, 10)) * 1000.0
    x = np.concatenate([centres[c] + rs.normal(size=(m, 10)) for c, m in enumerate(sizes)])
    member = np.repeat(np.arange(5), sizes)
    p = rs.permutation(len(x))
    return x[p], member[p]


def _approach(seed):
    x = _normal(seed, 1500, 4)
    return x[np.argsort(x[:, 0], kind="stable")]


def _duplicates(seed):
    x = _normal(seed, 300, 4)
    for lo, hi in ((7, 150), (40, 41), (299, 3)):                     # hi takes lo's row: three pairs of equal rows
        x[hi] = x[lo]
    return x


def _fixtures():
    f = collections.OrderedDict()

    def add(name, x, k, num_pcs=None, tied=False):
        f[name] = dict(x=np.ascontiguousarray(x, dtype=np.float64), k=k, num_pcs=num_pcs, tied=tied)

    add("two", _normal(101, 2, 3), 1)
    add("three", _normal(102, 3, 3), 2)
    add("n255", _normal(103, 255, 10), 64)
    add("n256", _normal(104, 256, 10), 64)
    add("n257", _normal(105, 257, 10), 64)
    add("n257_k256", _normal(105, 257, 10), 256)                      # every other row is a neighbour
    add("d1", _normal(106, 700, 1), 20)
    add("d3", _normal(107, 700, 3), 20)
    add("d128", _normal(108, 700, 128), 20)
    add("view", _normal(109, 600, 16), 30, num_pcs=10)
    add("rule_2000", _normal(110, 2000, 10), 166)
    add("clustered", _clustered(111)[0], 187)
    add("approach", _approach(112), 60)
    add("offset", 1e6 + _normal(113, 800, 6), 30)
    add("duplicates", _duplicates(114), 5, tied=True)
    add("lattice", np.random.RandomState(115).randint(0, 4, size=(200, 3)).astype(np.float64), 10, tied=True)
    add("mid_5000", _normal(116, 5000, 10), 214)
    return f


FIXTURES = _fixtures()
NOT_IN_GOLDEN = ("mid_5000",)
CLUSTERED_MEMBER = _clustered(111)[1]


def used(name):
    """the matrix the query sees: the first num_pcs columns, as a copy"""
    f = FIXTURES[name]
    return np.ascontiguousarray(f["x"][:, :f["num_pcs"]]) if f["num_pcs"] else f["x"]


_cache = {}


def expected(name):
    """the restatement of a fixture, computed once and shared: (indices, distances, d2); treat as read-only"""
    if name not in _cache:
        out = knn(used(name), FIXTURES[name]["k"])
        for a in out:
            a.setflags(write=False)
        _cache[name] = out
    return _cache[name]


def louvain_labels(num_barcodes, use_bcs, pairs):
    """load_louvain_results restated: the first line of a node wins, ids 1-based, 0 for a barcode that was not used"""
    labels = np.zeros(num_barcodes, dtype=np.int64)
    done = set()
    for node, community in pairs:
        if node not in done:
            done.add(node)
            labels[use_bcs[node]] = community + 1
    return labels
