"""CORRECT_CHEMISTRY_BATCH restated in plain numpy (no scikit-learn), and the fixtures of its tests.

The stage (mro/rna/stages/analyzer/correct_chemistry_batch/__init__.py, lib/python/cellranger/analysis/batch_correction.py):
  * split() puts the rows of a batch next to each other, the batches in id order, empty ids skipped;
  * find_knn(cur, ref, knn) = BallTree(ref).query(cur, knn): brute force it is the first knn pairs (d2, j) over the rows of ref, d2 =
    the sum over t of (x_t - y_t) * (x_t - y_t) in dimension order, f64, unfused, the lower index first among equal d2, NOTHING dropped;
  * join(): mutual_nn[(i, j)] = nn_ij & {(y, x) for x, y in nn_ji} with Python sets, overlap_percentage = the larger share of rows of i
    or of j that occur in a pair, align_orders = the pairs above alpha by descending overlap (sorted(..., reverse=True) is stable),
    the panorama loop, correction_vector per merge, x[cur] += corr;
  * correction_vector: w = exp(-(0.5 * sigma) * d2(x_c, x[mnn_cur[p]])), corr = (sum_p w b_p) / (sum_p w), b_p = x[mnn_ref[p]] -
    x[mnn_cur[p]].  HERE the sums run in a fixed order: the pairs in chunks of PAIR_CHUNK, left to right from 0.0 within a chunk, the
    chunks' partials left to right (include/crgpu.h); the reference's order is BLAS's and a Python set's.  The same code in
    np.longdouble (x86-64: 63 bits of mantissa, asserted) is the "exact" answer the f64 results are measured against;
  * batch_effect_score, with the neighbours by (d2, index).

FIXTURES: stage fixtures (a matrix and batch ids through the whole stage) and CORRECTIONS (one correction_vector call each).  Seeded,
small.  tests/golden/batch_correction_reference.npz (scripts/make_batch_correction_golden.py) holds the reference's own outputs.
"""
import collections

import numpy as np

PAIR_CHUNK = 2048      # CRGPU_BC_PAIR_CHUNK
KNN, ALPHA, SIGMA = 10, 0.1, 150.0

assert np.finfo(np.longdouble).nmant == 63, "the exact answers need the x87 extended format"


# ---- the neighbour query ------------------------------------------------------------------------------------------------------------
def d2_cross(x, q0, nq, c0, nc, dtype=np.float64):
    """[nq, nc]: the squared distances of the rows q0 .. to the rows c0 .., in dimension order, unfused"""
    x = np.asarray(x, dtype=dtype)
    acc = np.zeros((nq, nc), dtype)
    for t in range(x.shape[1]):
        diff = x[q0:q0 + nq, t][:, None] - x[None, c0:c0 + nc, t]
        acc += diff * diff
    return acc


def knn_cross(x, k, q0, nq, c0, nc):
    """-> (indices i32[nq, k] global, distances f64[nq, k], d2 f64[nq, k + 1] = the first k + 1 sorted d2 (k when nc == k))"""
    a = d2_cross(x, q0, nq, c0, nc)
    order = np.argsort(a, axis=1, kind="stable")                      # stable: the lower index first among equal d2
    d2 = np.take_along_axis(a, order[:, :k + 1], axis=1)
    return (order[:, :k] + c0).astype(np.int32), np.sqrt(d2[:, :k]), d2


# ---- split() and join() ---------------------------------------------------------------------------------------------------------------
def split(batch_ids, n_batch_ids=None):
    """-> (order = the rows in batch order, ranges [(lo, hi)], idx_to_batch_id, need_reorder)"""
    ids = np.asarray(batch_ids)
    nb = int(ids.max()) + 1 if n_batch_ids is None else n_batch_ids
    order, ranges, base = None, [], 0
    for b_id in range(nb):
        rows = np.where(ids == b_id)[0]
        if rows.shape[0] == 0:
            continue
        order = rows if order is None else np.append(order, rows)
        ranges.append((base, base + len(rows)))
        base += len(rows)
    return order, ranges, ids[order], not np.all(np.diff(order) >= 0)


def neighbours(x, ranges, k):
    """{(i, j): i32[n_i, k]}: main()'s find_knn of every ordered pair of batches, global indices"""
    return {(i, j): knn_cross(x, k, ranges[i][0], ranges[i][1] - ranges[i][0], ranges[j][0], ranges[j][1] - ranges[j][0])[0]
            for i in range(len(ranges)) for j in range(len(ranges)) if i != j}


def mutual(nn, ranges, k):
    """join()'s set arithmetic -> (mutual_nn {(i, j): set of (row of i, row of j)}, overlap {(i, j): float}), both in (i, j) order"""
    nn_pairs = {}
    for (i, j), ind in nn.items():
        left = np.repeat(np.arange(ranges[i][0], ranges[i][1]), k)
        nn_pairs[(i, j)] = set(zip(left.tolist(), ind.ravel().astype(int).tolist()))
    mutual_nn, overlap = collections.OrderedDict(), collections.OrderedDict()
    for i in range(len(ranges)):
        size_i = ranges[i][1] - ranges[i][0]
        for j in range(len(ranges)):
            if i >= j:
                continue
            nn_ij = nn_pairs[(i, j)]
            nn_ji = {(y, x) for x, y in nn_pairs[(j, i)]}
            mutual_nn[(i, j)] = nn_ij & nn_ji
            size_j = ranges[j][1] - ranges[j][0]
            overlap[(i, j)] = max(float(len({idx for idx, _ in mutual_nn[(i, j)]})) / size_i,
                                  float(len({idx for _, idx in mutual_nn[(i, j)]})) / size_j)
    return mutual_nn, overlap


def pairs_array(pair_set):
    """a set of pairs as i32[m, 2] in ascending order"""
    return np.array(sorted(pair_set), dtype=np.int32).reshape(-1, 2)


def schedule(ranges, mutual_nn, overlap, alpha=ALPHA, realign_panorama=False):
    """the panorama loop of join() without the arithmetic -> (align_orders, steps); a step = dict(ref_batches, cur_batches, cur_rows,
    mnn_cur, mnn_ref), the pairs in ascending (cur, ref) order"""
    align_orders = [k for k, v in sorted(overlap.items(), key=lambda kv: kv[1], reverse=True) if v > alpha]
    panoramas, count, steps = [], collections.defaultdict(int), []
    for i, j in align_orders:
        pi, pj = None, None
        for idx, panorama in enumerate(panoramas):
            if i in panorama:
                assert pi is None
                pi = idx
            if j in panorama:
                assert pj is None
                pj = idx
        if pi is None:
            panoramas.append({i})
            pi = len(panoramas) - 1
        if pj is None:
            panoramas.append({j})
            pj = len(panoramas) - 1
        if realign_panorama is True:
            count[i] += 1
            count[j] += 1
            if count[i] > 3 and count[j] > 3:
                continue
        elif pi == pj:
            continue
        size_i = sum(ranges[b][1] - ranges[b][0] for b in panoramas[pi])
        size_j = sum(ranges[b][1] - ranges[b][0] for b in panoramas[pj])
        if size_i < size_j:
            pi, pj = pj, pi
        cur_batches = sorted(panoramas[pj])
        cur_rows = np.concatenate([np.arange(ranges[b][0], ranges[b][1]) for b in cur_batches])
        matches = []
        for ref in panoramas[pi]:
            for cur in panoramas[pj]:
                if ref < cur and (ref, cur) in mutual_nn:
                    matches.extend([(c, r) for r, c in mutual_nn[(ref, cur)]])
                if ref > cur and (cur, ref) in mutual_nn:
                    matches.extend(mutual_nn[(cur, ref)])
        matches = pairs_array(matches)
        steps.append(dict(ref_batches=sorted(panoramas[pi]), cur_batches=cur_batches, cur_rows=cur_rows.astype(np.int32),
                          mnn_cur=np.ascontiguousarray(matches[:, 0]), mnn_ref=np.ascontiguousarray(matches[:, 1])))
        if pi != pj:
            panoramas[pi].update(panoramas[pj])
            panoramas.pop(pj)
    return align_orders, steps


# ---- correction_vector ------------------------------------------------------------------------------------------------------------------
def correction(x, cur_rows, mnn_cur, mnn_ref, sigma, dtype=np.float64, chunk=PAIR_CHUNK, want_den=False):
    """corr [n_cur, d] in `dtype`: the chunked sums of the header, every product and sum a rounding of its own (want_den: also den)"""
    x = np.asarray(x, dtype=dtype)
    cur_rows, mnn_cur, mnn_ref = (np.asarray(v, dtype=np.int64) for v in (cur_rows, mnn_cur, mnn_ref))
    neg_gamma = dtype(-(0.5 * sigma))
    xc = x[cur_rows]
    num, den = np.zeros(xc.shape, dtype), np.zeros(len(xc), dtype)
    for lo in range(0, len(mnn_cur), chunk):
        y = x[mnn_cur[lo:lo + chunk]]
        b = x[mnn_ref[lo:lo + chunk]] - y
        d2 = np.zeros((len(xc), len(y)), dtype)
        for t in range(x.shape[1]):
            diff = xc[:, t][:, None] - y[None, :, t]
            d2 += diff * diff
        w = np.exp(neg_gamma * d2)
        part_num, part_den = np.zeros(xc.shape, dtype), np.zeros(len(xc), dtype)
        for p in range(len(y)):
            part_num += w[:, p][:, None] * b[p][None, :]
            part_den += w[:, p]
        num += part_num
        den += part_den
    with np.errstate(invalid="ignore", divide="ignore"):
        corr = num / den[:, None]
    return (corr, den) if want_den else corr


def run_steps(x, steps, sigma, dtype=np.float64, permute=None):
    """the schedule applied in `dtype` -> (final matrix, [corr per step]); permute: None, or a function (step number, n_mnn) -> the order
    the pairs are taken in"""
    x = np.array(x, dtype=dtype)
    corrs = []
    for s, st in enumerate(steps):
        order = np.arange(len(st["mnn_cur"])) if permute is None else permute(s, len(st["mnn_cur"]))
        corr = correction(x, st["cur_rows"], st["mnn_cur"][order], st["mnn_ref"][order], sigma, dtype)
        x[st["cur_rows"]] += corr
        corrs.append(corr)
    return x, corrs


PAIR_ORDERS = collections.OrderedDict([
    ("ascending", None),
    ("reversed", lambda s, m: np.arange(m)[::-1]),
    ("permuted", lambda s, m: np.random.RandomState(777 + s).permutation(m)),
])


def max_abs(exact):
    """the largest finite |entry|: what a deviation is taken relative to"""
    exact = np.asarray(exact)
    ok = np.isfinite(exact)
    return float(np.abs(exact[ok]).max()) if ok.any() else 0.0


def rel_dev(got, exact, scale=None):
    """max |got - exact| over the entries that are finite in `exact`, relative to `scale` (default: the largest of those |exact|; a
    sample of rows is measured against the scale of the whole array); 0.0 when there is nothing to compare"""
    exact = np.asarray(exact)
    ok = np.isfinite(exact)
    if not ok.any():
        return 0.0
    scale = np.abs(exact[ok]).max() if scale is None else scale
    return float(np.abs(np.asarray(got, dtype=np.longdouble)[ok] - exact[ok]).max() / scale) if scale > 0 else 0.0


# ---- batch_effect_score -----------------------------------------------------------------------------------------------------------------
def knn_self(x, k):
    """the k entries after the first of every row's pairs (d2, index) over all rows: BallTree(x).query(x, k + 1)[:, 1:]
    -> (indices, d2 f64[n, k + 2] = the first k + 2 sorted d2, their indices)"""
    n = len(x)
    ind, d2, first = [], [], []
    for lo in range(0, n, 512):
        a = d2_cross(x, lo, min(512, n - lo), 0, n)
        order = np.argsort(a, axis=1, kind="stable")
        ind.append(order[:, 1:k + 1])
        first.append(order[:, :k + 2])
        d2.append(np.take_along_axis(a, order[:, :k + 2], axis=1))
    return np.concatenate(ind), np.concatenate(d2), np.concatenate(first)


def score_inputs(x, batch_ids, knn_neighbors=None, knn_frac=0.01, max_num_bcs=10000):
    """the subsample and k of batch_effect_score -> (x, ids, k), or None where the reference returns NaN"""
    x, ids = np.asarray(x), np.asarray(batch_ids)
    num_bcs, n_orig = len(x), len(set(ids.tolist()))
    if max_num_bcs is not None and num_bcs > max_num_bcs:
        select = np.random.RandomState(0).choice(num_bcs, max_num_bcs)
        select.sort()
        x, ids, num_bcs = x[select], ids[select], max_num_bcs
    counts = collections.Counter(ids.tolist())
    if len(counts) != n_orig or min(counts.values()) < 2:
        return None
    return x, ids, knn_neighbors if knn_neighbors is not None else int(np.ceil(knn_frac * num_bcs))


def batch_effect_score(x, batch_ids, knn_neighbors=None, knn_frac=0.01, max_num_bcs=10000):
    got = score_inputs(x, batch_ids, knn_neighbors, knn_frac, max_num_bcs)
    if got is None:
        return np.nan
    x, ids, k = got
    num_bcs = len(x)
    counts = collections.Counter(ids.tolist())
    num_batches = len(counts)
    to_frac = {b: (c - 1) / (num_bcs - 1) for b, c in counts.items()}
    null_frac = np.fromiter((to_frac[i] for i in ids.tolist()), dtype=np.float64)
    to_max = {b: min(c - 1, k) / k for b, c in counts.items()}
    max_frac = np.fromiter((to_max[i] for i in ids.tolist()), dtype=np.float64)
    knn_idx = knn_self(x, k)[0]
    same = np.mean(ids[:, None] == ids[knn_idx], axis=1)
    local = 1 + (num_batches - 1) * (same - null_frac) / (max_frac - null_frac)
    return float(np.mean(local))


# ---- the whole stage ----------------------------------------------------------------------------------------------------------------------
def stage(x, batch_ids, knn=KNN, alpha=ALPHA, sigma=SIGMA, realign_panorama=False, n_batch_ids=None, max_num_bcs=10000, dtype=np.float64,
          permute=None, scores=True):
    """-> dict(order, ranges, need_reorder, x = the reordered matrix, nn, mutual_nn (arrays), overlap, align_orders, steps, corr, final =
    the aligned matrix in batch order, aligned = in the input's order, score_before, score_after)"""
    order, ranges, ids, need_reorder = split(batch_ids, n_batch_ids)
    x = np.ascontiguousarray(np.asarray(x, dtype=np.float64)[order]) if need_reorder else np.asarray(x, dtype=np.float64)
    nn = neighbours(x, ranges, knn)
    mutual_nn, overlap = mutual(nn, ranges, knn)
    align_orders, steps = schedule(ranges, mutual_nn, overlap, alpha, realign_panorama)
    final, corr = run_steps(x, steps, sigma, dtype, permute)
    out = dict(order=order, ranges=ranges, ids=ids, need_reorder=need_reorder, x=x, nn=nn,
               mutual_nn=collections.OrderedDict((k, pairs_array(v)) for k, v in mutual_nn.items()), overlap=overlap, align_orders=align_orders,
               steps=steps, corr=corr, final=final, aligned=final[np.argsort(order)] if need_reorder else final)
    if scores:
        out["score_before"] = batch_effect_score(x, ids, max_num_bcs=max_num_bcs)
        out["score_after"] = batch_effect_score(np.asarray(final, dtype=np.float64), ids, max_num_bcs=max_num_bcs)
    return out


# ---- fixtures -----------------------------------------------------------------------------------------------------------------------------
def _batches(seed, d, noise, sizes, clusters, shift=0.05, spread=1.0):
    """rows of len(sizes) batches: batch b draws its rows evenly from the cluster centres clusters[b], plus a per-batch shift"""
    rs = np.random.RandomState(seed)
    centres = rs.normal(size=(1 + max(max(c) for c in clusters), d)) * spread
    offsets = rs.normal(size=(len(sizes), d)) * shift
    rows, ids = [], []
    for b, (m, cl) in enumerate(zip(sizes, clusters)):
        which = np.array(cl)[np.arange(m) % len(cl)]
        rows.append(centres[which] + offsets[b] + rs.normal(size=(m, d)) * noise)
        ids.append(np.full(m, b, np.int64))
    return np.concatenate(rows), np.concatenate(ids)


def _stage_fixtures():
    f = collections.OrderedDict()

    def add(name, x, ids, **kw):
        f[name] = dict(x=np.ascontiguousarray(x, dtype=np.float64), batch_ids=np.asarray(ids), knn=kw.pop("knn", KNN), alpha=kw.pop("alpha", ALPHA),
                       sigma=kw.pop("sigma", SIGMA), realign_panorama=kw.pop("realign_panorama", False), n_batch_ids=kw.pop("n_batch_ids", None),
                       max_num_bcs=kw.pop("max_num_bcs", 10000))
        assert not kw

    add("two_d10", *_batches(201, 10, 0.1, [300, 200], [[0, 1, 2], [0, 1, 2]]))
    add("three_d100", *_batches(202, 100, 0.03, [257, 130, 65], [[0, 1], [0, 1], [0, 1]], shift=0.01))
    # 0 and 2 share a cluster and merge first; the panorama {0, 2} is smaller than batch 1 and moves as two separate row ranges;
    # batch 3 shares a cluster with 1 alone: its overlaps with 0 and 2 stay below alpha
    add("four_panorama", *_batches(203, 10, 0.1, [300, 700, 250, 260], [[0], [0, 1, 1, 1, 1, 1], [0], [1, 2]], spread=3.0))
    x, ids = _batches(204, 10, 0.1, [150, 120, 90], [[0, 1], [0, 1], [0, 1]])
    p = np.random.RandomState(2040).permutation(len(x))
    add("interleaved", x[p], np.array([0, 2, 3])[ids[p]], n_batch_ids=5)        # ids 1 and 4 are empty
    add("far_apart", *_batches(205, 10, 0.05, [400, 300], [[0], [1]], spread=30.0), alpha=0.2)   # no overlap above alpha: nothing moves
    add("realign", *_batches(206, 10, 0.1, [160, 140, 120], [[0, 1], [0, 1], [0, 1]]), realign_panorama=True)
    add("score_subsample", *_batches(207, 10, 0.1, [420, 380], [[0, 1, 2], [0, 1, 2]]), max_num_bcs=500)
    return f


FIXTURES = _stage_fixtures()


def _corrections():
    f = collections.OrderedDict()

    def add(name, x, cur_rows, mnn_cur, mnn_ref, sigma=SIGMA):
        f[name] = dict(x=np.ascontiguousarray(x, dtype=np.float64), cur_rows=np.asarray(cur_rows, np.int32), mnn_cur=np.asarray(mnn_cur, np.int32),
                       mnn_ref=np.asarray(mnn_ref, np.int32), sigma=sigma)

    # more than two pair chunks with a ragged last one: 2 * 2048 + 609 pairs, drawn with repeats
    x, _ = _batches(301, 10, 0.1, [90, 80], [[0, 1], [0, 1]])
    rs = np.random.RandomState(3010)
    add("three_chunks", x, np.arange(90), rs.randint(0, 90, 2 * PAIR_CHUNK + 609), rs.randint(90, 170, 2 * PAIR_CHUNK + 609))
    # a cur row far from every pair: its weights underflow, 0 / 0
    x, _ = _batches(302, 10, 0.1, [70, 60], [[0], [0]])
    x[33] += 100.0
    rs = np.random.RandomState(3020)
    cur = rs.randint(0, 70, 300)
    add("nan_row", x, np.arange(70), np.where(cur == 33, 34, cur), rs.randint(70, 130, 300))
    x, _ = _batches(303, 7, 0.1, [40, 30], [[0], [0]])
    add("one_row_one_pair", x, [17], [5], [44])
    rs = np.random.RandomState(3040)
    add("one_row", x, [39], rs.randint(0, 40, 77), rs.randint(40, 70, 77))
    add("one_pair", x, np.arange(40), [11], [52])
    # d = 128, the largest; 33 rows: a row tile and one row
    x, _ = _batches(305, 128, 0.02, [33, 41], [[0], [0]], shift=0.01)
    rs = np.random.RandomState(3050)
    add("d128", x, np.arange(33), rs.randint(0, 33, 150), rs.randint(33, 74, 150))
    return f


CORRECTIONS = _corrections()

_cache = {}


def expected(name):
    """the f64 restatement of a stage fixture, computed once and shared; treat as read-only"""
    if name not in _cache:
        f = FIXTURES[name]
        _cache[name] = stage(f["x"], f["batch_ids"], f["knn"], f["alpha"], f["sigma"], f["realign_panorama"], f["n_batch_ids"], f["max_num_bcs"])
    return _cache[name]


def expected_correction(name):
    if ("c", name) not in _cache:
        f = CORRECTIONS[name]
        _cache[("c", name)] = correction(f["x"], f["cur_rows"], f["mnn_cur"], f["mnn_ref"], f["sigma"])
    return _cache[("c", name)]
