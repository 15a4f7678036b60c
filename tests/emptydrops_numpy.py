"""numpy / scipy restatement of the reference's EmptyDrops step, written for this project (it does not import the reference):

    find_nonambient_barcodes            lib/python/cellranger/cell_calling.py:144-263
    est_background_profile_sgt          cell_calling.py:47-102
    sgt_proportions                     sgt.py:24-132
    eval_multinomial_loglikelihoods     stats.py:24-46 (through scipy.special.gammaln)
    compute_ambient_pvalues             stats.py:205-231
    adjust_pvalue_bh                    analysis/diffexp.py:88-97

with the two rules this project sets where the reference is not reproducible (DESIGN.md "Cell calling"): ties of the ambient
range in stable order (np.argsort(kind="stable")[::-1]) and the simulation on a Philox4x64-10 stream (simulate_philox below).
It is the expected side of the GPU tests; tests/test_emptydrops_restatement.py pins it against the reference's recorded outputs
(tests/golden/emptydrops_reference.npz) and its Philox against numpy's."""
import numpy as np
from scipy.special import gammaln

STATUS_OK, STATUS_NO_AMBIENT, STATUS_SGT, STATUS_NO_CELLS, STATUS_NO_CANDIDATES = 0, 1, 2, 3, 4


class SimpleGoodTuringError(Exception):
    pass


# ---- Simple Good-Turing -------------------------------------------------------------------------------------------------------
def sgt_proportions(frequencies):
    """non-zero item frequencies -> (pstar, p0, slope); SimpleGoodTuringError for < 10 distinct frequencies or a slope > -1"""
    freq = np.asarray(frequencies, dtype=np.int64)
    assert len(freq) and (freq > 0).all()
    r, nr = np.unique(freq, return_counts=True)
    if len(r) < 10:
        raise SimpleGoodTuringError("too few distinct frequencies (%d)" % len(r))
    xr, xnr = r.astype(float), nr.astype(float)
    total = np.sum(xr * xnr)
    gap = np.concatenate(([1.0], np.diff(xr)))
    width = np.concatenate((0.5 * (gap[1:] + gap[:-1]), gap[-1:]))
    x, y = np.log(xr), np.log(xnr / width)
    slope = np.mean((x - x.mean()) * (y - y.mean())) / np.mean((x - x.mean()) ** 2)
    if slope > -1:
        err = SimpleGoodTuringError("log-log slope %g > -1" % slope)
        err.slope = slope
        raise err
    rel_lgt = xr * np.power(1 + 1.0 / xr, 1 + slope) / xr
    nxt_r, nxt_n = np.concatenate((xr[1:], [0.0])), np.concatenate((xnr[1:], [0.0]))
    turing = xr == nxt_r - 1
    rel_gt = np.zeros(len(xr))
    rel_gt[turing] = (xr[turing] + 1) / xr[turing] * nxt_n[turing] / xnr[turing]
    sd = np.ones(len(xr))
    idx = np.flatnonzero(turing)
    sd[idx] = (idx + 2.0) / xnr[idx] * np.sqrt(nxt_n[idx] * (1 + nxt_n[idx] / xnr[idx]))
    rel = np.zeros(len(xr))
    use_gt = True
    for k in range(len(xr)):
        if use_gt and np.abs(rel_lgt[k] - rel_gt[k]) * (1 + k) / sd[k] > 1.65:
            rel[k] = rel_gt[k]
        else:
            use_gt = False
            rel[k] = rel_lgt[k]
    raw = np.sum(rel * xr * xnr / total)
    p0 = xnr[0] / total
    rstar = xr * (rel * (1 - xnr[0] / total) / raw)
    rstar_sum = np.sum(xnr * rstar)
    pstar = (1 - p0) * (rstar[np.searchsorted(r, freq)] / rstar_sum)
    return pstar, p0, slope


# ---- the steps of find_nonambient_barcodes --------------------------------------------------------------------------------------
def column_sums(indptr, indices, data, n_features, mask=None):
    w = data.astype(np.int64) if mask is None else data.astype(np.int64) * (np.asarray(mask)[indices] != 0)
    cs = np.concatenate(([0], np.cumsum(w)))
    return (cs[indptr[1:]] - cs[indptr[:-1]]).astype(np.int64)


def row_sums(indptr, indices, data, n_features, cols=None, mask=None):
    if cols is None:
        idx, w = indices, data
    else:
        sel = np.concatenate([np.arange(indptr[c], indptr[c + 1]) for c in cols]) if len(cols) else np.zeros(0, np.int64)
        idx, w = indices[sel], data[sel]
    out = np.bincount(idx, weights=w.astype(np.float64), minlength=n_features).astype(np.int64)
    if mask is not None:
        out = out * (np.asarray(mask) != 0)
    return out


def ambient_set(umis, low, high):
    """(use_bcs ascending, max_background_umis): places [low, high) of the stable descending order, zero totals dropped"""
    empty = np.argsort(umis, kind="stable")[::-1][low:high]
    max_bg = int(np.max(umis[empty], initial=0))
    return np.sort(empty[umis[empty] > 0]), max_bg


def background_profile(indptr, indices, data, n_features, use_bcs, mask=None):
    """(eval_features, profile_p, p0, slope)"""
    eval_features = np.flatnonzero(row_sums(indptr, indices, data, n_features, None, mask))
    profile = row_sums(indptr, indices, data, n_features, use_bcs, mask)[eval_features]
    seen = np.flatnonzero(profile)
    pstar, p0, slope = sgt_proportions(profile[seen])
    n0 = len(profile) - len(seen)
    if n0 == 0:
        pstar = pstar / pstar.sum()
    profile_p = np.repeat(p0 / n0 if n0 else -1.0, len(profile))
    profile_p[seen] = pstar
    assert np.isclose(profile_p.sum(), 1.0)
    return eval_features, profile_p, p0, slope


def observed_loglk(indptr, indices, data, n_features, cols, eval_features, profile_p, mask=None):
    logp = np.zeros(n_features)
    logp[eval_features] = np.log(profile_p)
    keep = np.zeros(n_features, bool)
    keep[eval_features] = True
    if mask is not None:
        keep &= np.asarray(mask) != 0
    out = np.zeros(len(cols))
    for k, c in enumerate(cols):
        f, x = indices[indptr[c]:indptr[c + 1]], data[indptr[c]:indptr[c + 1]].astype(np.float64)
        ok = keep[f] & (x > 0)
        f, x = f[ok], x[ok]
        out[k] = gammaln(x.sum() + 1) + np.sum(x * logp[f] - gammaln(x + 1))
    return out


# ---- Philox4x64-10 and the device simulation --------------------------------------------------------------------------------------
_M32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def _mulhilo(a, b):
    """python int a (64 bits) x uint64 array b -> (hi, lo) uint64 arrays"""
    a_lo, a_hi = np.uint64(a & 0xFFFFFFFF), np.uint64(a >> 32)
    b_lo, b_hi = b & _M32, b >> _S32
    ll, lh, hl, hh = a_lo * b_lo, a_lo * b_hi, a_hi * b_lo, a_hi * b_hi
    mid = (ll >> _S32) + (lh & _M32) + (hl & _M32)
    hi = hh + (lh >> _S32) + (hl >> _S32) + (mid >> _S32)
    return hi, (mid << _S32) | (ll & _M32)


def philox_words(seed, s, n):
    """element t = 0 .. n-1: word t & 3 of Philox4x64-10(counter = (1 + (t >> 2), s, 0, 0), key = (seed, 0))"""
    nb = (n + 3) // 4
    c0 = np.arange(1, nb + 1, dtype=np.uint64)
    c1 = np.full(nb, s, dtype=np.uint64)
    c2, c3 = np.zeros(nb, np.uint64), np.zeros(nb, np.uint64)
    k0, k1 = int(seed) & (2 ** 64 - 1), 0
    with np.errstate(over="ignore"):
        for _ in range(10):
            hi0, lo0 = _mulhilo(0xD2E7470EE14C6C93, c0)
            hi1, lo1 = _mulhilo(0xCA5A826395121157, c2)
            c0, c1, c2, c3 = hi1 ^ c1 ^ np.uint64(k0), lo1, hi0 ^ c3 ^ np.uint64(k1), lo0
            k0 = (k0 + 0x9E3779B97F4A7C15) & (2 ** 64 - 1)
            k1 = (k1 + 0xBB67AE8584CAA73B) & (2 ** 64 - 1)
    return np.stack([c0, c1, c2, c3], axis=1).ravel()[:n]


def simulate_philox(profile_p, umis_per_bc, num_sims, seed=0):
    """the device simulation: (distinct_n, loglk[len(distinct_n), num_sims]).  The counts of simulation s at N are its first N
    draws; loglk = lgamma(N + 1) + sum over the draws of log p_j - log(count of j before the draw + 1), which is
    lgamma(N + 1) + sum_j (c_j log p_j - lgamma(c_j + 1)).  The running sum is kept in extended precision."""
    distinct_n = np.flatnonzero(np.bincount(umis_per_bc))
    distinct_n = distinct_n[distinct_n > 0]
    nmax = int(distinct_n[-1])
    cdf = np.cumsum(profile_p)
    cdf = cdf / cdf[-1]
    logp = np.log(profile_p)
    lg = gammaln(distinct_n + 1.0)
    out = np.zeros((len(distinct_n), num_sims))
    ar = np.arange(nmax)
    for s in range(num_sims):
        u = (philox_words(seed, s, nmax) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
        feat = np.searchsorted(cdf, u, side="right")
        order = np.argsort(feat, kind="stable")
        sf = feat[order]
        start = np.flatnonzero(np.concatenate(([True], sf[1:] != sf[:-1])))
        before = np.empty(nmax, np.int64)
        before[order] = ar - np.repeat(start, np.diff(np.concatenate((start, [nmax]))))
        run = np.cumsum((logp[feat] - np.log(before + 1.0)).astype(np.longdouble))
        out[:, s] = lg + run[distinct_n - 1].astype(np.float64)
    return distinct_n, out


# ---- p-values, BH ---------------------------------------------------------------------------------------------------------------
def count_lower(umis_per_bc, obs_loglk, sim_n, sim_loglk):
    rows = np.searchsorted(sim_n, umis_per_bc)
    return np.array([np.sum(sim_loglk[rows[i]] < obs_loglk[i]) for i in range(len(umis_per_bc))], dtype=np.int64)


def ambient_pvalues(umis_per_bc, obs_loglk, sim_n, sim_loglk):
    return (1 + count_lower(umis_per_bc, obs_loglk, sim_n, sim_loglk)).astype(float) / (1 + sim_loglk.shape[1])


def adjust_pvalue_bh(p):
    descending = np.argsort(p)[::-1]
    scale = float(len(p)) / np.arange(len(p), 0, -1)
    q = np.minimum(1, np.minimum.accumulate(scale * p[descending]))
    return q[np.argsort(descending)]


def find_nonambient(indptr, indices, data, n_features, cell_cols, low, high, minimum_umis=500, num_sims=10000, max_adj_pvalue=0.01,
                    seed=0, mask=None, sim_table=None):
    """-> dict: status and, as far as the step got, n_ambient_used, max_background_umis, emptydrops_minimum_umis, eval_features,
    profile_p, eval_cols, umis, obs_loglk, sim_n, sim_loglk, n_lower, pvalues, pvalues_adj, is_nonambient, called_cols"""
    umis_per_bc = column_sums(indptr, indices, data, n_features, mask)
    cell_cols = np.asarray(cell_cols, dtype=np.int64)
    r = {"status": STATUS_OK, "called_cols": cell_cols.copy()}
    use_bcs, max_bg = ambient_set(umis_per_bc, low, high)
    r.update(n_ambient_used=len(use_bcs), max_background_umis=max_bg, emptydrops_minimum_umis=max(minimum_umis, 1 + max_bg))
    if len(use_bcs) == 0:
        return dict(r, status=STATUS_NO_AMBIENT)
    try:
        ef, p, p0, slope = background_profile(indptr, indices, data, n_features, use_bcs, mask)
    except SimpleGoodTuringError:
        return dict(r, status=STATUS_SGT)
    r.update(eval_features=ef, profile_p=p, sgt_p0=p0, sgt_slope=slope)
    if len(cell_cols) == 0:
        return dict(r, status=STATUS_NO_CELLS)
    cand = umis_per_bc >= r["emptydrops_minimum_umis"]
    cand[cell_cols] = False
    eval_cols = np.flatnonzero(cand)
    if len(eval_cols) == 0:
        return dict(r, status=STATUS_NO_CANDIDATES)
    umis = umis_per_bc[eval_cols]
    obs = observed_loglk(indptr, indices, data, n_features, eval_cols, ef, p, mask)
    sim_n, sim_loglk = sim_table if sim_table is not None else simulate_philox(p, umis, num_sims, seed)
    n_lower = count_lower(umis, obs, sim_n, sim_loglk)
    pvalues = (1 + n_lower).astype(float) / (1 + sim_loglk.shape[1])
    adj = adjust_pvalue_bh(pvalues)
    call = adj <= max_adj_pvalue
    r.update(eval_cols=eval_cols, umis=umis, obs_loglk=obs, sim_n=np.asarray(sim_n), sim_loglk=sim_loglk, n_lower=n_lower, pvalues=pvalues,
             pvalues_adj=adj, is_nonambient=call, called_cols=np.union1d(cell_cols, eval_cols[call]))
    return r


def near_tie(obs_loglk, umis, sim_n, sim_loglk, rel=1e-9):
    """a simulated value within `rel` of the observed one it is compared with: n_lower may then differ by rounding alone"""
    rows = np.searchsorted(sim_n, umis)
    return bool(np.any(np.abs(sim_loglk[rows] - obs_loglk[:, None]) <= rel * np.abs(obs_loglk[:, None])))


# ---- the fixture well -------------------------------------------------------------------------------------------------------------
def make_well(seed, n_features=600,n_cells=200, n_ambient=4000, n_big_ambient=150, n_small_cells=60):
    """CSC of a planted well in random column order (np.random.RandomState: one stream for all numpy versions):
    cells with log-normal totals and small cells of 150 - 599 UMIs from profile A; ambient droplets of 1 - 99 and large ambient
    droplets of 150 - 599 UMIs from profile B.  -> (indptr, indices, data, n_features, kind[V]) with kind 0 = cell, 1 = ambient,
    2 = large ambient, 3 = small cell"""
    rs = np.random.RandomState(seed)
    # log-normal expression levels: the ambient row sums then have the falling frequency-of-frequency curve SGT asks for
    pa, pb = np.exp(rs.normal(0, 2, n_features)), np.exp(rs.normal(0, 2, n_features))
    pa, pb = pa / pa.sum(), pb / pb.sum()
    totals = np.concatenate([np.maximum(2000, rs.lognormal(np.log(6000), 0.5, n_cells)).astype(np.int64),
                             rs.randint(1, 100, n_ambient), rs.randint(150, 600, n_big_ambient), rs.randint(150, 600, n_small_cells)])
    kind = np.repeat([0, 1, 2, 3], [n_cells, n_ambient, n_big_ambient, n_small_cells])
    perm = rs.permutation(len(totals))
    totals, kind = totals[perm], kind[perm]
    indptr, idx, dat = [0], [], []
    for t, k in zip(totals, kind):
        c = rs.multinomial(t, pa if k in (0, 3) else pb)
        nz = np.flatnonzero(c)
        idx.append(nz)
        dat.append(c[nz])
        indptr.append(indptr[-1] + len(nz))
    return (np.array(indptr, np.int64), np.concatenate(idx).astype(np.int32), np.concatenate(dat).astype(np.int32), n_features, kind)


FIXTURE = dict(low=1000, high=3000, minimum_umis=100, fdr=0.01)
