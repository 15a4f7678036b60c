"""Plain numpy restatement of the aggregate stage and the two closing cell filters, written from the description of the stage
(include/crgpu.h, "protein aggregates"), not from the reference's text:

  * signal antibodies = antibody rows with a sum >= 1000 over all columns; fewer than 5: nothing is found
  * K = 25 * max(num_probe_barcodes, 1); candidates = the top K columns by their sum over the signal rows
  * a candidate is an aggregate when it is among the top K columns of at least int(np.round(n_signal * frac)) signal rows, implicit
    zeros taking part; frac = 0.6 for n_signal > 26, else -0.02 * n_signal + 1.1
  * highly corrected: reads > 10000 and corrected / reads > 0.5
  * antigen outliers: the top min(100, V) columns by their antigen sum, q1 / q3 = np.quantile of those sums, threshold = q3 + (q3 - q1)
    * 3; below 1000 nothing, else the columns of the top with a sum >= threshold
  * minimum UMIs: cells with a sum >= minimum; mitochondrial: cells with 100.0 * mt / total > max leave, NaN stays

"The top n" is taken under a TIE RULE, the one thing the reference leaves open (numpy's default sort is unstable): "high" = among equal
values the higher column wins (np.argsort(x, kind="stable")[-n:], the library's rule), "low" = the lower column wins.  A fixture whose
result is the same under both rules is tie-insensitive: whatever order the reference's sort produced, it gives that result.

The closing filters' reference functions live in cellranger/cell_calling_helpers.py, whose import pulls in the pipeline's own compiled
packages; it cannot be imported outside the pipeline, so their cases in tests/test_aggregates_restatement.py are computed by hand.
"""
import numpy as np

KIND_OTHER, KIND_ANTIBODY, KIND_ANTIGEN = 0, 1, 2
COUNTS, HIGHLY_CORRECTED, ANTIGEN = 1, 2, 4
SIGNAL_UMIS, TOP_UMI_BCS, NUM_READS, ANTIGEN_TOP, ANTIGEN_MIN = 1000, 25, 10000, 100, 1000
AB, AG = "Antibody Capture", "Antigen Capture"


def fraction_to_use(n_signal):
    return 0.6 if n_signal > 26 else -0.02 * n_signal + 1.1


def min_antibodies(n_signal):
    return int(np.round(n_signal * fraction_to_use(n_signal)))


def top_n(x, n, tie="high"):
    """the positions of the n largest values of x; among equal values at the boundary the higher ("high") or lower ("low") position wins"""
    x = np.asarray(x)
    if n <= 0:
        return np.zeros(0, np.int64)
    pos = np.arange(len(x))
    order = np.lexsort((pos if tie == "high" else -pos, x))      # ascending by value, then by +-position
    return order[-n:]


def dense_rows(indptr, indices, data, n_features, rows):
    """the rows `rows` of the CSC matrix as a dense i64 array [len(rows), V]"""
    V = len(indptr) - 1
    at = np.full(n_features, -1, np.int64)
    at[rows] = np.arange(len(rows))
    out = np.zeros((len(rows), V), np.int64)
    col = np.repeat(np.arange(V), np.diff(indptr))
    sel = at[indices] >= 0
    np.add.at(out, (at[indices[sel]], col[sel]), data[sel].astype(np.int64))
    return out


def column_sums(indptr, indices, data, mask):
    V = len(indptr) - 1
    col = np.repeat(np.arange(V), np.diff(indptr))
    sel = np.asarray(mask)[indices] != 0
    return np.bincount(col[sel], weights=data[sel].astype(np.float64), minlength=V).astype(np.int64)      # sums < 2^53


def aggregates_by_counts(indptr, indices, data, n_features, kind, num_probe_barcodes=None, tie="high"):
    """-> (the aggregate columns ascending, dict(n_antibodies, n_signal, top_k, n_candidates, min_antibodies))"""
    kind = np.asarray(kind)
    V = len(indptr) - 1
    ab = np.flatnonzero(kind == KIND_ANTIBODY)
    K = TOP_UMI_BCS * max(int(num_probe_barcodes or 0), 1)
    info = dict(n_antibodies=len(ab), n_signal=0, top_k=K, n_candidates=0, min_antibodies=0)
    none = np.zeros(0, np.uint64)
    if V == 0:
        return none, info
    table = dense_rows(indptr, indices, data, n_features, ab)
    table = table[table.sum(axis=1) >= SIGNAL_UMIS]
    n_signal = len(table)
    info.update(n_signal=n_signal, min_antibodies=min_antibodies(n_signal))
    if n_signal < 5:
        return none, info
    cand = top_n(table.sum(axis=0), K, tie)
    info["n_candidates"] = len(cand)
    votes = np.zeros(V, np.int64)
    for row in table:
        votes[top_n(row, K, tie)] += 1
    found = np.sort(cand[votes[cand] >= info["min_antibodies"]])
    return found.astype(np.uint64), info


def highly_corrected(reads, corrected):
    reads, corrected = np.asarray(reads, np.float64), np.asarray(corrected, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        high = (corrected / reads > 0.5) & (reads > NUM_READS)
    return np.flatnonzero(high).astype(np.uint64)


def antigen_threshold(top_counts):
    x = np.asarray(top_counts, np.int64)
    q3, q1 = np.quantile(x, 0.75), np.quantile(x, 0.25)
    return q1, q3, q3 + (q3 - q1) * 3


def antigen_outliers(indptr, indices, data, n_features, kind, tie="high"):
    """-> (columns ascending, threshold or None for an empty matrix)"""
    V = len(indptr) - 1
    if V == 0:
        return np.zeros(0, np.uint64), None
    counts = column_sums(indptr, indices, data, np.asarray(kind) == KIND_ANTIGEN)
    top = top_n(counts, min(ANTIGEN_TOP, V), tie)
    threshold = antigen_threshold(counts[top])[2]
    if threshold < ANTIGEN_MIN:
        return np.zeros(0, np.uint64), threshold
    return np.sort(top[counts[top] >= threshold]).astype(np.uint64), threshold


def select_barcodes(indptr, indices, data, cols):
    cols = np.asarray(cols, np.int64)
    lens = indptr[cols + 1] - indptr[cols]
    new_ptr = np.zeros(len(cols) + 1, np.int64)
    np.cumsum(lens, out=new_ptr[1:])
    take = np.concatenate([np.arange(indptr[c], indptr[c + 1]) for c in cols]) if len(cols) else np.zeros(0, np.int64)
    return new_ptr, indices[take], data[take]


def remove_aggregates(fx, tie="high"):
    """the union on a fixture dict (indptr, indices, data, n_features, kind, num_probe_barcodes, reads / corrected: {library type: per
    column} or None) -> dict(removed, reasons, kept, info, antigen_threshold, libraries)"""
    indptr, indices, data, nf, kind = fx["indptr"], fx["indices"], fx["data"], fx["n_features"], np.asarray(fx["kind"])
    V = len(indptr) - 1
    reasons = np.zeros(V, np.uint8)
    reads, corrected = fx.get("reads") or {}, fx.get("corrected") or {}
    info, thr, bits = None, None, {}
    if (kind == KIND_ANTIBODY).any():
        bits[AB] = (COUNTS | HIGHLY_CORRECTED, KIND_ANTIBODY)
        if AB in reads and AB in corrected:
            reasons[highly_corrected(reads[AB], corrected[AB]).astype(np.int64)] |= HIGHLY_CORRECTED
        cols, info = aggregates_by_counts(indptr, indices, data, nf, kind, fx.get("num_probe_barcodes"), tie)
        reasons[cols.astype(np.int64)] |= COUNTS
    if (kind == KIND_ANTIGEN).any():
        bits[AG] = (ANTIGEN, KIND_ANTIGEN)
        cols, thr = antigen_outliers(indptr, indices, data, nf, kind, tie)
        reasons[cols.astype(np.int64)] |= ANTIGEN
    removed = np.flatnonzero(reasons).astype(np.uint64)
    libraries = {}
    for lib, (mask, k) in bits.items():
        cols = removed[(reasons[removed.astype(np.int64)] & mask) != 0].astype(np.int64)
        d = dict(number_aggregate_GEMs=len(cols), cols=cols.astype(np.uint64), reads_removed=None, reads_total=None,
                 umis=column_sums(indptr, indices, data, kind == k)[cols])
        if lib in reads:
            r = np.asarray(reads[lib], np.int64)
            d.update(reads=r[cols], reads_removed=int(r[cols].sum()), reads_total=int(r.sum()))
            if lib in corrected:
                d["corrected_reads"] = np.asarray(corrected[lib], np.int64)[cols]
        libraries[lib] = d
    return dict(removed=removed, reasons=reasons[removed.astype(np.int64)], kept=np.flatnonzero(reasons == 0).astype(np.uint64), info=info,
                antigen_threshold=thr, libraries=libraries)


def apply_minimum_umis(cols, umis, minimum_umis):
    cols = np.asarray(cols, np.int64)
    return cols[np.asarray(umis, np.int64)[cols] >= minimum_umis].astype(np.uint64)


def apply_mito_threshold(cols, mito_umis, total_umis, max_mito_percent):
    """-> (kept columns, removed columns, their total UMIs, their mt_pct)"""
    cols = np.asarray(cols, np.int64)
    mt, tot = np.asarray(mito_umis, np.int64)[cols], np.asarray(total_umis, np.int64)[cols]
    with np.errstate(divide="ignore", invalid="ignore"):
        pct = 100.0 * mt / tot
    out = pct > max_mito_percent
    return cols[~out].astype(np.uint64), cols[out].astype(np.uint64), tot[out], pct[out]


# ---- fixtures ----------------------------------------------------------------------------------------------------------------------
def from_dense(dense, kind, **kw):
    """a fixture from a dense [n_features, V] array (CSC, rows ascending, explicit zeros dropped)"""
    dense = np.asarray(dense, np.int64)
    nf, V = dense.shape
    f, c = np.nonzero(dense.T)[::-1]      # column-major: sorted by column, then by row
    indptr = np.zeros(V + 1, np.int64)
    np.cumsum(np.bincount(c, minlength=V), out=indptr[1:])
    fx = dict(indptr=indptr, indices=f.astype(np.int32), data=dense[f, c].astype(np.int32), n_features=nf, kind=np.asarray(kind, np.uint8),
              num_probe_barcodes=None, reads=None, corrected=None)
    fx.update(kw)
    return fx


def random_well(seed, n_ab=None, V=None, num_probe_barcodes=None, n_gex=6, n_ag=2, interleave=False):
    """Poisson background of every antibody over every barcode, cells that stain a subset of the panel, a handful of planted aggregates
    that are high in nearly all antibodies, an antigen library with a few outliers, and a read table whose corrected share is high in a
    few barcodes"""
    rng = np.random.RandomState(seed)
    n_ab = int(rng.randint(4, 30)) if n_ab is None else n_ab
    V = int(rng.randint(200, 3001)) if V is None else V
    kind = np.array([KIND_OTHER] * n_gex + [KIND_ANTIBODY] * n_ab + [KIND_ANTIGEN] * n_ag, np.uint8)
    if interleave:
        kind = kind[rng.permutation(len(kind))]
    dense = np.zeros((len(kind), V), np.int64)
    ab, ag, gex = (np.flatnonzero(kind == k) for k in (KIND_ANTIBODY, KIND_ANTIGEN, KIND_OTHER))
    dense[gex] = rng.poisson(0.5, (len(gex), V))
    lam = rng.choice([0.05, 0.3, 1.0, 3.0, 8.0], n_ab)
    dense[ab] = rng.poisson(lam[:, None], (n_ab, V))
    cells = rng.choice(V, V // 8, replace=False)
    for c in cells:
        on = rng.rand(n_ab) < 0.3
        dense[ab[on], c] += rng.poisson(60, int(on.sum()))
    planted = rng.choice(V, int(rng.randint(0, 7)), replace=False)
    for c in planted:
        on = rng.rand(n_ab) < 0.9
        dense[ab[on], c] += rng.poisson(rng.choice([400, 1500]), int(on.sum()))
    dense[ag] = rng.poisson(4.0, (len(ag), V))
    for c in rng.choice(V, int(rng.choice([0, 45])), replace=False):      # antigen binders: without them the threshold stays below 1000
        dense[ag, c] += rng.poisson(400, len(ag))
    for c in rng.choice(V, int(rng.randint(0, 4)), replace=False):
        dense[ag, c] += rng.poisson(2500, len(ag))
    reads = (dense[ab].sum(axis=0) * 3 + rng.poisson(5, V)).astype(np.int64)
    corrected = rng.binomial(reads, 0.05)
    for c in rng.choice(V, 3, replace=False):
        reads[c] += 12000
        corrected[c] = int(reads[c] * 0.7)
    ag_reads = (dense[ag].sum(axis=0) * 2).astype(np.int64)
    return from_dense(dense, kind, num_probe_barcodes=num_probe_barcodes, reads={AB: reads, AG: ag_reads}, corrected={AB: corrected}, seed=seed,
                      planted=np.sort(planted))


GOLDEN_SEEDS = ((101, None), (102, None), (103, 2), (104, None), (105, 1), (106, 2), (107, None), (108, None))


def golden_fixtures():
    """the seeded wells that scripts/make_aggregates_golden.py records the reference's outputs for (it asserts that each of them is
    tie-insensitive); num_probe_barcodes None, 1 and 2"""
    return [("well%d" % seed, random_well(seed, num_probe_barcodes=npb)) for seed, npb in GOLDEN_SEEDS]
