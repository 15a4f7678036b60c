"""RUN_GRAPH_CLUSTERING's Louvain restated in numpy, in the synchronous integer round form include/crgpu.h states for
csrc/louvain.hip (no GPU).

The reference carries no source of bin/louvain and bin/convert; this file is the published algorithm (Blondel et al. 2008) in a round
form whose every quantity is an integer: a round is a pure function of the labels at its start, every comparison is exact and every
sum is order-independent, so the device equals this file bit for bit.  No parity with the binary is claimed.

A graph is (indptr i64[n + 1], indices, weights): a symmetric CSR with ascending columns, a diagonal entry counted once.
singleton_rule=False drops the rule that keeps two singletons from swapping places; it exists for the test that shows the rule is
under test and is no part of the contract.
"""
import numpy as np

MAX_ROUNDS = 1000
MAX_LEVELS = 64
LIMIT = 1 << 31


def csr_rows(indptr):
    indptr = np.asarray(indptr, dtype=np.int64)
    return np.repeat(np.arange(len(indptr) - 1, dtype=np.int64), np.diff(indptr))


def from_keys(keys, weights, n):
    """sorted distinct keys i * n + j -> (indptr, indices, weights)"""
    indptr = np.searchsorted(keys, np.arange(n + 1, dtype=np.int64) * n).astype(np.int64)
    return indptr, (keys % n).astype(np.int64), np.asarray(weights, dtype=np.int64)


def union(indptr, indices):
    """symmetrize = 1: A_ij = A_ji = 1 when j is in row i or i is in row j, A_ii = 1 when i is in row i, duplicates collapse"""
    n = len(indptr) - 1
    rows, cols = csr_rows(indptr), np.asarray(indices, dtype=np.int64)
    keys = np.unique(np.concatenate([rows * n + cols, cols * n + rows]))
    return from_keys(keys, np.ones(len(keys), dtype=np.int64), n)


def check_symmetric(indptr, indices, weights):
    """symmetrize = 0: ascending columns without duplicates, weights >= 1 and equal in both directions"""
    n = len(indptr) - 1
    rows, cols, w = csr_rows(indptr), np.asarray(indices, dtype=np.int64), np.asarray(weights, dtype=np.int64)
    if len(cols) and (cols.min() < 0 or cols.max() >= n):
        raise ValueError("an index outside the nodes")
    keys = rows * n + cols
    if np.any(np.diff(keys) <= 0):
        raise ValueError("the columns of a row must be strictly ascending")
    if np.any(w < 1):
        raise ValueError("a weight below 1")
    back = cols * n + rows
    at = np.searchsorted(keys, back)
    ok = at < len(keys)
    ok[ok] &= keys[at[ok]] == back[ok]
    if not ok.all() or np.any(w[at] != w):
        raise ValueError("the graph is not symmetric")


def int_bincount(idx, w, n):
    out = np.zeros(n, dtype=np.int64)
    np.add.at(out, idx, w)
    return out


def degrees(graph):
    """k_i = sum_j A_ij with the diagonal counted once, M = sum_i k_i"""
    indptr, _, w = graph
    k = int_bincount(csr_rows(indptr), w, len(indptr) - 1)
    return k, int(k.sum())


def modularity_S(graph, labels):
    """-> (S, M): S = sum_C (in_C * M - tot_C^2), Q = S / M^2"""
    indptr, cols, w = graph
    c = np.asarray(labels, dtype=np.int64)
    rows = csr_rows(indptr)
    k, M = degrees(graph)
    inside = int(w[c[rows] == c[cols]].sum())
    tot = int_bincount(c, k, int(c.max()) + 1 if len(c) else 0)
    return inside * M - int((tot * tot).sum()), M


def one_round(graph, k, M, c, singleton_rule=True):
    """-> (c', surviving proposals), everything read from c"""
    indptr, cols, w = graph
    n = len(indptr) - 1
    rows = csr_rows(indptr)
    tot, size = int_bincount(c, k, n), np.bincount(c, minlength=n)
    off = rows != cols
    # the candidates of node i: its own community (weight 0 from this line) and the community of every neighbour j != i
    node = np.concatenate([np.arange(n, dtype=np.int64), rows[off]])
    comm = np.concatenate([c, c[cols[off]]])
    wt = np.concatenate([np.zeros(n, dtype=np.int64), w[off]])
    uk, inv = np.unique(node * n + comm, return_inverse=True)
    w_iC = int_bincount(inv, wt, len(uk))
    ci, cc = uk // n, uk % n
    own = cc == c[ci]
    G = w_iC * M - (tot[cc] - np.where(own, k[ci], 0)) * k[ci]
    order = np.lexsort((cc, ~own, -G, ci))       # per node: the largest (G, C == own, -C) first
    first = np.ones(len(order), dtype=bool)
    first[1:] = ci[order][1:] != ci[order][:-1]
    best = cc[order][first]
    move = best != c
    if singleton_rule:
        move &= ~((size[c] == 1) & (size[best] == 1) & (best > c))
    return np.where(move, best, c), int(move.sum())


def run_level(graph, max_rounds=MAX_ROUNDS, singleton_rule=True):
    """-> (labels, counted rounds, S of the labels)"""
    n = len(graph[0]) - 1
    k, M = degrees(graph)
    c = np.arange(n, dtype=np.int64)
    S, rounds = modularity_S(graph, c)[0], 0
    while rounds < max_rounds:
        c2, moved = one_round(graph, k, M, c, singleton_rule)
        if not moved:
            break
        S2 = modularity_S(graph, c2)[0]
        if S2 <= S:
            break
        c, S, rounds = c2, S2, rounds + 1
    return c, rounds, S


def renumber(c):
    """dense labels in ascending order of community id -> (dense, communities)"""
    ids, dense = np.unique(c, return_inverse=True)
    return dense.astype(np.int64), len(ids)


def aggregate(graph, dense, n_c):
    """A'_CD = sum_{c_i = C, c_j = D} A_ij"""
    indptr, cols, w = graph
    rows = csr_rows(indptr)
    keys, inv = np.unique(dense[rows] * n_c + dense[cols], return_inverse=True)
    return from_keys(keys, int_bincount(inv, w, len(keys)), n_c)


def louvain(indptr, indices, weights=None, symmetrize=True, max_rounds=MAX_ROUNDS, singleton_rule=True):
    """-> dict(levels: list of i64[nodes of the level], nodes, communities, rounds, S: lists per level, M, level0, final)"""
    indptr = np.asarray(indptr, dtype=np.int64)
    n = len(indptr) - 1
    if not 1 <= n < LIMIT:
        raise ValueError("1 <= n < 2^31")
    if symmetrize:
        if weights is not None:
            raise ValueError("symmetrize = 1 takes no weights")
        cols = np.asarray(indices, dtype=np.int64)
        if len(cols) and (cols.min() < 0 or cols.max() >= n):
            raise ValueError("an index outside the nodes")
        graph = union(indptr, indices)
    else:
        weights = np.ones(len(indices), dtype=np.int64) if weights is None else np.asarray(weights, dtype=np.int64)
        check_symmetric(indptr, indices, weights)
        graph = (indptr, np.asarray(indices, dtype=np.int64), weights)
    M = degrees(graph)[1]
    if not 1 <= M < LIMIT:
        raise ValueError("1 <= M < 2^31")
    out = dict(levels=[], nodes=[], communities=[], rounds=[], S=[], M=M)
    comp = np.arange(n, dtype=np.int64)
    while len(out["levels"]) < MAX_LEVELS:
        c, rounds, S = run_level(graph, max_rounds, singleton_rule)
        if rounds == 0 and out["levels"]:
            break
        dense, n_c = renumber(c)
        out["levels"].append(dense)
        out["nodes"].append(len(c)), out["communities"].append(n_c), out["rounds"].append(rounds), out["S"].append(S)
        comp = dense[comp]
        if len(out["levels"]) == 1:
            out["level0"] = comp.copy()
        if rounds == 0:
            break
        graph = aggregate(graph, dense, n_c)
        assert degrees(graph)[1] == M
    out["final"] = comp
    return out


def pairs(result):
    """the (node, community) lines of `louvain -l -1`: every level in turn"""
    return [(i, int(c)) for level in result["levels"] for i, c in enumerate(level)]


def csr_from_edges(n, edges, weights=None):
    """undirected edges (i, j) (a self-loop once) -> a symmetric CSR (symmetrize = 0 input)"""
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    w = np.ones(len(e), dtype=np.int64) if weights is None else np.asarray(weights, dtype=np.int64)
    loop = e[:, 0] == e[:, 1]
    keys = np.concatenate([e[:, 0] * n + e[:, 1], e[~loop, 1] * n + e[~loop, 0]])
    ww = np.concatenate([w, w[~loop]])
    order = np.argsort(keys, kind="stable")
    return from_keys(keys[order], ww[order], n)


def directed_csr(n, edges):
    """edges as given, row by row in ascending column order: a symmetrize = 1 input"""
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    order = np.lexsort((e[:, 1], e[:, 0]))
    e = e[order]
    indptr = np.searchsorted(e[:, 0], np.arange(n + 1)).astype(np.int64)
    return indptr, e[:, 1].astype(np.int32)


# ---- the hand-computed cases ------------------------------------------------------------------------------------------------------------
def hand_cases():
    """name -> (n, edges, expected final labels or None, expected (S, M) or None)"""
    return {
        "two_triangles": (6, [(0, 1), (0, 2), (1, 2), (3, 4), (3, 5), (4, 5), (2, 3)], [0, 0, 0, 1, 1, 1], (70, 14)),
        "one_edge": (2, [(0, 1)], [0, 0], None),
        "star8": (9, [(0, i) for i in range(1, 9)], [0] * 9, None),
        "path4": (4, [(0, 1), (1, 2), (2, 3)], [0, 0, 1, 1], (6, 6)),
        "k4": (4, [(i, j) for i in range(4) for j in range(i + 1, 4)], [0] * 4, None),
        "self_loop": (3, [(0, 0), (0, 1), (1, 2)], [0, 1, 1], (2, 5)),
    }


def ring(n, perm=None):
    p = np.arange(n) if perm is None else np.asarray(perm)
    return [(int(p[i]), int(p[(i + 1) % n])) for i in range(n)]


def hub_rows(n):
    """a kNN-like directed graph in which every row names node 0 (the hub) and its successor: a symmetrize = 1 input"""
    edges = [(i, 0) for i in range(1, n)] + [(i, (i + 1) % n) for i in range(n)] + [(i, (i + 7) % n) for i in range(0, n, 3)]
    edges = sorted(set(e for e in edges if e[0] != e[1]))
    return directed_csr(n, edges)


def three_groups(seed, rows=100, dims=10):
    """row r of group g: randn plus 10 on coordinate g"""
    x = np.random.RandomState(seed).randn(3 * rows, dims)
    for g in range(3):
        x[g * rows:(g + 1) * rows, g] += 10.0
    return x


def knn_csr(x, k):
    """the neighbour matrix of run_graph_clustering: the k nearest rows of every row (the row itself left out), row-wise ascending"""
    import knn_numpy

    ind = np.sort(knn_numpy.knn(x, k)[0], axis=1)
    return np.arange(len(x) + 1, dtype=np.int64) * k, ind.reshape(-1).astype(np.int32)


def blobs(seed, sizes, dims=10, spread=4.0):
    rs = np.random.RandomState(seed)
    centres = rs.normal(size=(len(sizes), dims)) * spread
    return np.concatenate([centres[g] + rs.normal(size=(s, dims)) for g, s in enumerate(sizes)])


def golden_fixtures():
    """name -> (indptr, indices): the kNN graphs the golden file records networkx's serial Louvain on"""
    import collections

    f = collections.OrderedDict()
    for seed in (0, 1, 2):
        for k in (15, 67):
            f["groups_s%d_k%d" % (seed, k)] = knn_csr(three_groups(seed), k)
    f["blobs600_k20"] = knn_csr(blobs(5, [200, 150, 120, 80, 50]), 20)
    f["normal500_k20"] = knn_csr(np.random.RandomState(9).normal(size=(500, 10)), 20)
    f["blobs2000_k35"] = knn_csr(blobs(6, [700, 500, 400, 250, 150], spread=2.0), 35)
    return f
