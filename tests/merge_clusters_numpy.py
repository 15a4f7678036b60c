"""MERGE_CLUSTERS restated in numpy: the specification of csrc/sseq_pair.h, csrc/merge_clusters.hip and engine.merge_clusters (include/crgpu.h
has the same text).  It follows join() of mro/rna/stages/analyzer/merge_clusters/__init__.py statement by statement; the sSeq test is
tests/sseq_numpy.py (no parity with the diff_exp crate, whose source was not available).

pair_columns(groups, a, b)          the cells of the groups listed in a in (group, cell) order, then those of b
compare(x, groups, a, b)            sseq_numpy.compute_params + diffexp on x[:, cols] with the labels 1 .. 1, 2 .. 2, cluster 1
cluster_medians(pca, labels, K)     np.median of every column over the rows of every cluster
linkage_complete(points)            scipy's linkage(points, "complete") as a plain Lance-Williams loop; ties by the smallest (height, id0, id1)
merge_clusters(x, pca, labels)      the stage loop -> the dict of engine.merge_clusters (without the times)
FIXTURES / fixture(name, bump)      the seeded wells; bump = seeds to skip (the recorder replaces a rejected fixture)"""
import numpy as np

import sseq_numpy as S

DE_THRESHOLD = 0.05      # MERGE_CLUSTERS_DE_ADJ_P_THRESHOLD


def pair_columns(groups, a, b):
    """groups: i32[cells], -1 = in no group -> (cols, n_a)"""
    groups = np.asarray(groups)
    ca = [np.flatnonzero(groups == g) for g in a]
    cb = [np.flatnonzero(groups == g) for g in b]
    return np.concatenate(ca + cb), int(sum(len(c) for c in ca))


def compare(x, groups, a, b, de_threshold=DE_THRESHOLD, want_p=True):
    """-> dict: the parameters of the pair's cells, cluster 1 of the two-label test, n_de, min_q = the smallest adjusted p"""
    cols, na = pair_columns(groups, a, b)
    sub = np.asarray(x)[:, cols]
    labels = np.array([1] * na + [2] * (len(cols) - na), np.int32)
    P = S.compute_params(sub)
    o = S.diffexp(sub, P, labels, 2, want_p=want_p)
    r = dict(cols=cols, n_cells_a=na, n_cells_b=len(cols) - na, zeta_hat=P["zeta_hat"], delta=P["delta"], n_used=P["n_used"], use=P["use_g"],
             mean=P["mean_g"], phi_mm=P["phi_mm_g"], phi=P["phi_g"], s_a=o["s_a"][0], s_b=o["s_b"][0], sums_a=o["sums_in"][0], sums_b=o["sums_out"][0],
             norm_mean_a=o["norm_mean_in"][0], norm_mean_b=o["norm_mean_out"][0], log2_fold_change=o["log2_fold_change"][0], p_values=o["p_values"][0],
             adjusted_p_values=o["adjusted_p_values"][0], below_median=o["below_median"][0], n_exact=int(o["n_exact"][0]),
             n_asymptotic=int(o["n_asymptotic"][0]), min_gap=o["min_gap"][0], median=o["median"][0])
    r["n_terms"] = int(sum(int(r["sums_a"][g]) + int(r["sums_b"][g]) + 1 for g in np.flatnonzero(r["use"]) if r["below_median"][g] == 255))
    thr = DE_THRESHOLD if de_threshold == 0 else de_threshold
    r["n_de"] = int(np.sum(r["adjusted_p_values"] < thr))
    r["min_q"] = float(r["adjusted_p_values"].min())
    return r


def cluster_medians(pca, labels, n_clusters=None):
    pca, labels = np.asarray(pca, np.float64), np.asarray(labels)
    K = int(labels.max()) + 1 if n_clusters is None else int(n_clusters)
    return np.array([np.median(pca[labels == c], axis=0) for c in range(K)])


def linkage_complete(points):
    """-> Z f64[K - 1, 4]: the greedy agglomeration, the pair with the smallest (height, id0, id1) first"""
    pts = np.asarray(points, np.float64)
    K, d = pts.shape
    D = np.zeros((K, K))
    for t in range(d):      # the sum of squares in dimension order
        e = pts[:, t][:, None] - pts[:, t][None, :]
        D += e * e
    D = np.sqrt(D)
    ids, size = list(range(K)), [1] * K
    live = list(range(K))
    Z = np.zeros((K - 1, 4))
    for step in range(K - 1):
        best = None
        for ii, i in enumerate(live):
            for j in live[ii + 1:]:
                key = (D[i, j], min(ids[i], ids[j]), max(ids[i], ids[j]), i, j)
                if best is None or key[:3] < best[:3]:
                    best = key
        h, id0, id1, i, j = best
        a, b = (i, j) if ids[i] < ids[j] else (j, i)
        Z[step] = (id0, id1, h, size[a] + size[b])
        live.remove(b)
        for k in live:
            if k != a:
                D[a, k] = D[k, a] = max(D[a, k], D[b, k])
        size[a] += size[b]
        ids[a] = K + step
    return Z


def relabel_by_size(labels):
    labels = np.asarray(labels)
    by_size = np.argsort(-np.bincount(labels), kind="stable")
    rank = np.empty(len(by_size), dtype=np.int64)
    rank[by_size] = np.arange(len(by_size))
    return 1 + rank[labels]


def merge_clusters(x, pca, labels, de_threshold=DE_THRESHOLD, medians=cluster_medians, linkage=linkage_complete, test=None, trace=None):
    """x int[G, barcodes], pca f64[barcodes, PCs], labels 1-based with 0 = not used -> dict(labels, steps, n_tests, n_skipped, n_merges,
    n_iterations, n_clusters_in, n_clusters_out).  medians / linkage / test can be replaced (the recorder passes pandas, scipy and the
    stage's cell order); trace, a list, receives (medoids, Z) of every iteration and min_q of every test"""
    labels = np.asarray(labels)
    use_bcs = np.flatnonzero(labels > 0)
    lab = labels[use_bcs].astype(np.int64) - 1
    n_in = int(lab.max()) + 1
    sub_pca = np.asarray(pca, np.float64)[use_bcs]
    groups = np.full(len(labels), -1, np.int64)
    groups[use_bcs] = lab
    if test is None:
        def test(a, b, cells0, cells1):
            return compare(x, groups, a, b, de_threshold)
    members = [[g] for g in range(n_in)]
    steps, checked = [], set()
    n_tests = n_skipped = n_merges = n_iterations = 0
    while len(members) > 1:
        n_iterations += 1
        medoids = medians(sub_pca, lab, len(members))
        hc = linkage(medoids)
        if trace is not None:
            trace.append(("iteration", np.array(medoids), np.array(hc)))
        max_label = len(members) - 1
        any_merged = False
        for step in range(hc.shape[0]):
            if not (hc[step, 0] <= max_label and hc[step, 1] <= max_label):
                continue
            leaf0, leaf1 = int(hc[step, 0]), int(hc[step, 1])
            rec = dict(iteration=n_iterations, leaf0=leaf0, leaf1=leaf1, groups0=list(members[leaf0]), groups1=list(members[leaf1]), skipped=False,
                       n_de=None, merged=False)
            steps.append(rec)
            key = frozenset((frozenset(members[leaf0]), frozenset(members[leaf1])))
            if key in checked:
                rec["skipped"] = True
                n_skipped += 1
                continue
            checked.add(key)
            r = test(members[leaf0], members[leaf1], use_bcs[lab == leaf0], use_bcs[lab == leaf1])
            if trace is not None:
                trace.append(("test", r["min_q"], r["adjusted_p_values"]))
            n_tests += 1
            rec["n_de"] = r["n_de"]
            if r["n_de"] == 0:
                lab[lab == leaf1] = leaf0
                lab[lab > leaf1] -= 1
                members[leaf0] = sorted(members[leaf0] + members[leaf1])
                del members[leaf1]
                rec["merged"] = any_merged = True
                n_merges += 1
                break
        if not any_merged:
            break
    final = np.zeros(len(labels), dtype=np.int64)
    final[use_bcs] = relabel_by_size(lab + 1)
    return dict(labels=final, steps=steps, n_tests=n_tests, n_skipped=n_skipped, n_merges=n_merges, n_iterations=n_iterations, n_clusters_in=n_in,
                n_clusters_out=len(members))


STEP_FIELDS = ("iteration", "leaf0", "leaf1", "skipped", "n_de", "merged")


def steps_table(steps):
    """the step log as an i64 table (n_de of a skipped pair: -1) and the initial groups of both leaves as one flat list with offsets"""
    tab = np.array([[s["iteration"], s["leaf0"], s["leaf1"], int(s["skipped"]), -1 if s["n_de"] is None else s["n_de"], int(s["merged"])] for s in steps],
                   np.int64).reshape(-1, len(STEP_FIELDS))
    flat, off = [], [0]
    for s in steps:
        for k in ("groups0", "groups1"):
            flat += list(s[k])
            off.append(len(flat))
    return tab, np.array(flat, np.int64), np.array(off, np.int64)


# ---- fixtures ----------------------------------------------------------------------------------------------------------------------------
G, PCS = 80, 5
FIXTURES = {
    "oversplit": dict(seed=201),
    "distinct": dict(seed=202),
    "all_one": dict(seed=203),
    "cached_pair": dict(seed=204),
    "unused_barcodes": dict(seed=205),
    "small_clusters": dict(seed=206),
    "wide": dict(seed=207),
}


def _well(rs, sizes, centers, sd=1.0, n_marker=20, fold=4.0):
    """planted groups: negative-binomial counts with `n_marker` genes a group raised `fold` times, a Gaussian cloud of `sd` around the
    group's centre in PCS dimensions -> (x int64[G, N], pca f64[N, PCS], truth i64[N]), the cells shuffled"""
    truth = np.repeat(np.arange(len(sizes)), sizes)
    rs.shuffle(truth)
    N = len(truth)
    base = np.exp(rs.uniform(np.log(0.2), np.log(6.0), G))
    effect = np.ones((G, len(sizes)))
    for k in range(len(sizes)):
        effect[rs.choice(G, n_marker, replace=False), k] = fold
    depth = np.exp(rs.normal(0.0, 0.3, N))
    mu = base[:, None] * depth[None, :] * effect[:, truth]
    r = 1.0 / rs.uniform(0.1, 0.8, G)[:, None]
    x = rs.negative_binomial(r, r / (r + mu)).astype(np.int64)
    x[0, x.sum(axis=0) == 0] = 1      # no empty cell
    sd = np.broadcast_to(np.asarray(sd, np.float64), (len(sizes),))
    pca = np.asarray(centers, np.float64)[truth] + rs.normal(0.0, 1.0, (N, PCS)) * sd[truth][:, None]
    return x, pca, truth


def _split(rs, truth, parts):
    """every planted group k cut at random into parts[k] labels -> 1-based labels"""
    labels, nxt = np.zeros(len(truth), np.int64), 1
    for k, p in enumerate(parts):
        cells = np.flatnonzero(truth == k)
        labels[cells] = nxt + np.concatenate([np.arange(p), rs.randint(0, p, len(cells) - p)])[rs.permutation(len(cells))]
        nxt += p
    return labels


def _centers(rs, n, scale):
    return rs.normal(0.0, scale, (n, PCS))


def fixture(name, bump=0):
    """-> (x int64[G, barcodes], pca f64[barcodes, PCS], labels i64[barcodes], 1-based, 0 = not used)"""
    rs = np.random.RandomState(FIXTURES[name]["seed"] + 1000 * bump)
    if name == "oversplit":      # 3 groups, each split at random in two
        x, pca, truth = _well(rs, [140, 120, 180], _centers(rs, 3, 8.0))
        return x, pca, _split(rs, truth, [2, 2, 2])
    if name == "distinct":       # 4 groups in two tight pairs
        c = np.zeros((4, PCS))
        c[:, 0] = [0.0, 4.0, 30.0, 35.0]
        x, pca, truth = _well(rs, [80, 110, 60, 140], c)
        return x, pca, truth + 1
    if name == "all_one":        # one group in 4 labels
        x, pca, truth = _well(rs, [200], np.zeros((1, PCS)))
        return x, pca, _split(rs, truth, [4])
    if name == "cached_pair":    # two distinct groups 1.0 apart in PC 1, a third far away split by the sign of PC 3
        c = np.zeros((3, PCS))
        c[:, 0] = [0.0, 1.0, 40.0]
        x, pca, truth = _well(rs, [100, 120, 160], c, sd=[0.2, 0.2, 1.0])
        labels = truth + 1
        labels[(truth == 2) & (pca[:, 2] > 0)] = 4
        return x, pca, labels
    if name == "unused_barcodes":   # every third label 0
        x, pca, truth = _well(rs, [150, 180, 210], _centers(rs, 3, 8.0))
        labels = _split(rs, truth, [2, 1, 2])
        labels[::3] = 0
        return x, pca, labels
    if name == "small_clusters":    # clusters of 1 and 2 cells beside two large ones
        c = np.zeros((4, PCS))
        c[:, 0] = [0.0, 25.0, 60.0, 61.0]
        x, pca, truth = _well(rs, [90, 70, 1, 2], c, sd=[1.0, 1.0, 0.1, 0.1])
        return x, pca, truth + 1
    if name == "wide":           # 17 initial clusters of 4 groups
        x, pca, truth = _well(rs, [300, 240, 260, 280], _centers(rs, 4, 10.0))
        return x, pca, _split(rs, truth, [5, 4, 4, 4])
    raise KeyError(name)
