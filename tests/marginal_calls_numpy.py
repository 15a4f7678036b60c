"""The marginal caller restated in numpy, in two forms that must agree: CELL order (the dense vector of one feature, as the reference
hands it to scikit-learn) and HISTOGRAM order (the distinct values of a sparse row with their multiplicities, the zeros one bin, as
csrc/marginal_calls.h runs it).  Written from the behaviour of call_presence_with_gmm_ab under scikit-learn 1.7.2
(GaussianMixture(n_components=2, n_init=10, covariance_type="tied", random_state=0)); no text of either is used.

One fit:
  draws      RandomState(0) anew per feature; init j takes one double (the first centre: the cell where the running sum of 1/V,
             divided by its last value, first exceeds it) and two more (the trial candidates)
  seeding    on x - mean(x): potential = sum of squared distances to the first centre; each trial draw u * potential is located in
             the running sum of those distances in cell order (first cell whose running sum reaches it, clipped to the last cell);
             the candidate whose min-distance potential is smaller becomes the second centre, the first on a tie
  Lloyd      labels to the nearer centre (tie: centre 0), centres = means, an empty cluster keeps its centre; stop when the labels
             repeat (they stand), or when the squared shift is <= 1e-4 var(x) or after 300 rounds (then one relabel)
  EM         from the one-hot labels: nk + 10 eps, means, tied covariance + 1e-6, weights nk / n; then e-step / m-step with the lower
             bound = mean log-sum-exp under the previous parameters until |change| < 1e-3, at most 100 times; weights renormalised
  winner     the first init, then any later one with a strictly larger lower bound
  calls      count >= umi_threshold and argmax of the weighted log probabilities == argmax of the means (ties: the first)
A row whose maximum is 0, or with fewer than 2 cells, is not fitted."""
import numpy as np

N_INIT = 10
EPS10 = 10 * np.finfo(np.float64).eps
LOG_2PI = np.log(2 * np.pi)
SKLEARN_VERSION = "1.7.2"


def seed_draws(V):
    """-> (u f64[10, 3], first_cell i64[10]): what every feature's fit draws; it depends on V alone"""
    rs = np.random.RandomState(0)
    u = np.zeros((N_INIT, 3))
    for j in range(N_INIT):
        u[j, 0] = rs.random_sample()
        u[j, 1:] = rs.random_sample(2)
    cdf = np.cumsum(np.full(V, 1.0 / V))
    cdf /= cdf[-1]
    first = np.minimum(np.searchsorted(cdf, u[:, 0], side="right"), V - 1)
    return u, first.astype(np.int64)


def _nearer_to_second(xc, c0, c1):
    return np.abs(xc - c1) < np.abs(xc - c0)


def _lloyd(xc, m, c0, c1, tol, diag):
    p0 = p1 = None
    repeat = False
    for it in range(300):
        lab = _nearer_to_second(xc, c0, c1)
        diag["midpoints"].append(0.5 * (c0 + c1))
        n1, n0 = m[lab].sum(), m[~lab].sum()
        new0 = (m[~lab] * xc[~lab]).sum() / n0 if n0 > 0 else c0
        new1 = (m[lab] * xc[lab]).sum() / n1 if n1 > 0 else c1
        same = it > 0 and np.array_equal(lab, _nearer_to_second(xc, p0, p1))
        shift = (new0 - c0) ** 2 + (new1 - c1) ** 2
        f0, f1 = c0, c1
        p0, p1 = c0, c1
        c0, c1 = new0, new1
        if same:
            repeat = True
            break
        if shift <= tol:
            break
    if not repeat:
        f0, f1 = c0, c1
        diag["midpoints"].append(0.5 * (c0 + c1))
    return _nearer_to_second(xc, f0, f1)


def _log_prob(xv, w, mu, pc):
    y = xv[:, None] * pc - mu[None, :] * pc
    return -0.5 * (LOG_2PI + y * y) + np.log(pc) + np.log(w)[None, :]


def _em(xv, m, n, lab, diag):
    xx = ((m * xv) * xv).sum()
    r = np.zeros((len(xv), 2))
    r[np.arange(len(xv)), lab.astype(int)] = 1.0

    def m_step(r, first):
        mr = m[:, None] * r
        nk = mr.sum(0) + EPS10
        mu = (mr * xv[:, None]).sum(0) / nk
        nks = nk[0] + nk[1]
        cov = (xx - ((nk[0] * mu[0]) * mu[0] + (nk[1] * mu[1]) * mu[1])) / nks + 1e-6
        if first:
            w = nk / n
        else:
            w = nk / nks
            w = w / (w[0] + w[1])
        return w, mu, cov

    w, mu, cov = m_step(r, True)
    lb = -np.inf
    n_iter = 0
    for n_iter in range(1, 101):
        prev = lb
        pc = 1.0 / np.sqrt(cov)
        a = _log_prob(xv, w, mu, pc)
        mx = a.max(1)
        lse = np.log(np.exp(a[:, 0] - mx) + np.exp(a[:, 1] - mx)) + mx
        r = np.exp(a - lse[:, None])
        w, mu, cov = m_step(r, False)
        lb = (m * lse).sum() / n
        diag["stop_margin"] = min(diag["stop_margin"], abs(abs(lb - prev) - 1e-3))
        if abs(lb - prev) < 1e-3:
            break
    return w, mu, cov, lb, n_iter


def _finish(fits, vals, xv, umi_threshold, diag):
    win = 0
    for j in range(1, len(fits)):
        if fits[j][3] > fits[win][3]:
            win = j
    w, mu, cov, lb, n_iter = fits[win]
    a = _log_prob(xv, w, mu, 1.0 / np.sqrt(cov))
    pred = (a[:, 1] > a[:, 0]).astype(int)
    pos = int(mu[1] > mu[0])
    on = (pred == pos) & (vals >= umi_threshold)
    if mu[0] != mu[1]:
        diag["boundary"] = (mu[0] ** 2 - mu[1] ** 2 - 2 * cov * (np.log(w[0]) - np.log(w[1]))) / (2 * (mu[0] - mu[1]))
    hi, lo = pos, 1 - pos
    return dict(fitted=True, winner=win, n_iter=n_iter, lower_bound=lb, covariance=cov, mean_low=mu[lo], mean_high=mu[hi], weight_low=w[lo],
                weight_high=w[hi], lower_bounds=np.array([f[3] for f in fits]), n_iters=np.array([f[4] for f in fits])), on


def _skipped(n):
    return dict(fitted=False, calls=np.zeros(n, bool), cells_assigned=0, umi_threshold_observed=-1, winner=-1, n_iter=0)


def _new_diag():
    return dict(midpoints=[], stop_margin=np.inf, boundary=np.nan, mean=0.0, landings=[], first_is_entry=[])


def fit_dense(counts, umi_threshold=1, draws=None):
    """cell order: counts i64[V] of one feature -> dict(calls bool[V], parameters, diag)"""
    counts = np.asarray(counts, np.int64)
    V = len(counts)
    if V < 2 or counts.max() == 0:
        return _skipped(V)
    u, first = draws if draws is not None else seed_draws(V)
    x = np.log10(1 + counts)
    mean = x.mean()
    xc = x - mean
    m = np.ones(V)
    tol = 1e-4 * np.var(x)
    diag = _new_diag()
    diag["mean"] = mean
    fits = []
    for j in range(N_INIT):
        c0 = xc[first[j]]
        d = (xc - c0) ** 2
        pot = d.sum()
        cand = np.minimum(np.searchsorted(np.cumsum(d), u[j, 1:] * pot), V - 1)
        pots = [np.minimum(d, (xc - xc[k]) ** 2).sum() for k in cand]
        c1 = xc[cand[1]] if pots[1] < pots[0] else xc[cand[0]]
        lab = _lloyd(xc, m, c0, c1, tol, diag)
        fits.append(_em(x, m, float(V), lab, diag))
    res, on = _finish(fits, counts, x, umi_threshold, diag)
    res.update(calls=on, cells_assigned=int(on.sum()), umi_threshold_observed=int(counts[on].min()) if on.any() else -1, diag=diag)
    return res


def row_histogram(V, cols, vals):
    """the distinct values of a sparse row, ascending, with their multiplicities; the zeros are one bin of V - nnz"""
    dv, mult = np.unique(np.asarray(vals, np.int64), return_counts=True)
    if len(cols) < V:
        dv, mult = np.concatenate(([0], dv)), np.concatenate(([V - len(cols)], mult))
    return dv.astype(np.int64), mult.astype(np.int64)


def _locate(r, cols, de, d0, V, vals):
    """the first cell whose running squared distance, in cell order, reaches r: entry e stands behind gap_e zeros.  -> (its value,
    where it lies: 0 among the zeros before the first entry, 1 in a later gap, 2 on an entry, 3 behind the last entry)"""
    n = len(cols)
    if n == 0:
        return 0, 3
    gaps = np.diff(np.concatenate(([-1], cols))) - 1
    s = np.cumsum(gaps * d0 + de)
    g = s - de
    hit_gap = (gaps > 0) & (r <= g)
    hit_ent = r <= s
    any_hit = hit_gap | hit_ent
    if any_hit.any():
        e = int(np.argmax(any_hit))
        return (0, 0 if e == 0 else 1) if hit_gap[e] else (int(vals[e]), 2)
    return (0, 3) if cols[-1] + 1 < V else (int(vals[-1]), 2)


def fit_histogram(V, cols, vals, umi_threshold=1, draws=None):
    """histogram order: a sparse row (cols ascending, vals > 0) over V cells -> the same dict as fit_dense; calls bool[nnz] per entry"""
    cols, vals = np.asarray(cols, np.int64), np.asarray(vals, np.int64)
    if V < 2 or len(vals) == 0:
        return _skipped(len(vals))
    u, first = draws if draws is not None else seed_draws(V)
    dv, mult = row_histogram(V, cols, vals)
    xv, m, n = np.log10(1 + dv), mult.astype(np.float64), float(V)
    mean = (m * xv).sum() / n
    xvc = xv - mean
    tol = 1e-4 * ((m * (xvc * xvc)).sum() / n)
    xe = np.log10(1 + vals) - mean
    diag = _new_diag()
    diag["mean"] = mean
    fits = []
    for j in range(N_INIT):
        at = np.searchsorted(cols, first[j])
        v0 = int(vals[at]) if at < len(cols) and cols[at] == first[j] else 0
        c0 = np.log10(1 + v0) - mean
        dh = (xvc - c0) ** 2
        pot = (m * dh).sum()
        d0 = (0.0 - mean - c0) ** 2
        de = (xe - c0) ** 2
        where = [_locate(u[j, t] * pot, cols, de, d0, V, vals) for t in (1, 2)]
        cv = [w[0] for w in where]
        diag["landings"] += [w[1] for w in where]
        diag["first_is_entry"].append(v0 > 0)
        cc = [np.log10(1 + v) - mean for v in cv]
        pots = [(m * np.minimum(dh, (xvc - c) ** 2)).sum() for c in cc]
        c1 = cc[1] if pots[1] < pots[0] else cc[0]
        lab = _lloyd(xvc, m, c0, c1, tol, diag)
        fits.append(_em(xv, m, n, lab, diag))
    res, on_v = _finish(fits, dv, xv, umi_threshold, diag)
    on = on_v[np.searchsorted(dv, vals)]
    res.update(calls=on, cells_assigned=int(on.sum()), umi_threshold_observed=int(vals[on].min()) if on.any() else -1, diag=diag, values=dv,
               multiplicities=mult)
    return res


def identify_contaminants(counts, order, min_counts=1000, dynamic_range=50.0, max_cor=0.5):
    """counts i64[n_tags, V] -> (flags u8[n]: 0 kept, 1 contaminant, 2 dropped for zero UMIs; sources: per tag the list of its source
    tags in the order met).  order: the tags sorted by id, as a permutation."""
    counts = np.asarray(counts, np.int64)
    k, V = counts.shape
    tot = counts.sum(1)
    flags = np.zeros(k, np.uint8)
    for t in range(k):
        if tot[t] == 0:
            flags[t] = 2
        elif tot[t] < min_counts or tot[t] * dynamic_range < tot.max():
            flags[t] = 1
    src = [[] for _ in range(k)]
    live = [int(t) for t in order if flags[t] != 2]
    for a in range(len(live) - 1):
        for b in range(a + 1, len(live)):
            i, j = live[a], live[b]
            sx, sy = int(tot[i]), int(tot[j])
            sxx, syy, sxy = int((counts[i] * counts[i]).sum()), int((counts[j] * counts[j]).sum()), int((counts[i] * counts[j]).sum())
            vx, vy, cxy = V * sxx - sx * sx, V * syy - sy * sy, V * sxy - sx * sy
            if vx <= 0 or vy <= 0:
                continue                                  # a NaN correlation
            if cxy / (np.sqrt(float(vx)) * np.sqrt(float(vy))) < max_cor:
                continue
            loser, other = (i, j) if tot[i] < tot[j] else (j, i)
            flags[loser] = 1
            src[loser].append(other)
    return flags, src


def umi_interval_snr(counts, threshold):
    """_get_umi_interval and the log10_snr column of _compute_umi_thresholds, rounded to 3 places"""
    counts = np.asarray(counts)
    noise, signal = counts[counts < threshold], counts[counts >= threshold]
    q3 = np.percentile(noise, 75) if len(noise) else 0
    q1 = np.percentile(signal, 25) if len(signal) else 0
    return float(np.round(np.log10(q1 + 1) - np.log10(q3 + 1), 3))


def margins_ok(res, x_values, margin=1e-9):
    """True when integers and iteration counts of a fit do not hang on the last bits: no init's stopping difference | |change| - 1e-3 |
    is below `margin`, and no Lloyd midpoint and not the winner's decision boundary lies within `margin` of a data value (x_values: the
    distinct log10(1 + count) of the row).  A row of ONE distinct value over all cells is exempt from the midpoint half: both centres
    ARE that value, the tie rule decides its labels, and either outcome gives the same calls and the same low / high parameters."""
    d = res["diag"]
    if d["stop_margin"] < margin:
        return False
    x_values = np.asarray(x_values, np.float64)
    pts = np.array(d["midpoints"]) + d["mean"] if len(x_values) > 1 else np.zeros(0)
    if np.isfinite(d["boundary"]):
        pts = np.append(pts, d["boundary"])
    return bool(np.all(np.abs(pts[:, None] - x_values[None, :]) > margin))
