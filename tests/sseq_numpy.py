"""The sSeq differential expression of clusters restated in numpy and scipy: the specification of csrc/sseq.h (include/crgpu.h has the
same text).  It follows Yu et al. 2013 as the pure-Python diffexp.py of open-source Cell Ranger 3 had it; the reference tree's stage
takes its numerics from the external diff_exp crate, whose source was not available, so no parity with that crate is claimed.

compute_params(x)                          compute_sseq_params: size factors, mean_g, var_g, use_g, phi_mm_g, zeta_hat, delta, phi_g
diffexp(x, params, labels, n_clusters)     sseq_differential_expression of every cluster against all other cells
adjust_bh(p)                               adjust_pvalue_bh
*_mp                                       the same quantities in exact arithmetic (mpmath, 40 digits) from the integer matrix on
FIXTURES / fixture(name, bump)             the seeded test matrices; bump = seeds to skip (the recorder replaces a rejected fixture)

`order` picks one of three orders of every sum over cells (numpy's pairwise sum, ascending, descending): the recorder stores how far
the parameters and means move between them."""
import numpy as np
from scipy import special, stats

BIG_COUNT = 900
ZETA_QUANTILE = 0.995


def _sum(a, order=0):
    """the sum over the last axis in one of three orders"""
    a = np.asarray(a, dtype=np.float64)
    if order == 0:
        return np.sum(a, axis=-1)
    if order == 1:
        return np.cumsum(a, axis=-1)[..., -1]
    return np.cumsum(a[..., ::-1], axis=-1)[..., -1]


def compute_params(x, order=0):
    """x: int array [G, N] -> dict; ValueError where the device refuses"""
    x = np.asarray(x)
    G, N = x.shape
    if G < 3 or N < 2:
        raise ValueError("G >= 3 and N >= 2")
    counts = x.sum(axis=0)
    med = np.median(counts)
    if counts.min() == 0 or med == 0:
        raise ValueError("a cell without counts")
    sf = counts.astype(np.float64) / med
    xn = x / sf
    mean = _sum(xn, order) / N
    mean_sq = _sum(xn * xn, order) / N
    var = mean_sq - mean * mean
    use = var > 0
    if not use.any():
        raise ValueError("no used gene")
    S = _sum(1.0 / sf, order)
    phi_mm = np.zeros(G)
    phi_mm[use] = np.maximum(0.0, (N * var[use] - mean[use] * S) / (mean[use] * mean[use] * S))
    zeta_hat = np.nanpercentile(phi_mm[use], 100 * ZETA_QUANTILE)
    any_pos = bool(np.any(phi_mm[use] > 0))
    num = np.sum(np.square(phi_mm[use] - np.mean(phi_mm[use]))) / float(G - 1)
    den = np.sum(np.square(phi_mm[use] - zeta_hat)) / float(G - 2)
    if any_pos and not den > 0:
        raise ValueError("delta is x / 0")
    delta = num / den if any_pos else np.nan
    phi = np.full(G, np.nan)
    phi[use] = (1 - delta) * phi_mm[use] + delta * zeta_hat if any_pos else 0.0
    return dict(size_factors=sf, mean_g=mean, var_g=var, use_g=use, phi_mm_g=phi_mm, phi_g=phi, zeta_hat=float(zeta_hat), delta=float(delta),
                n_used=int(use.sum()))


def _lp(k, m, f):
    if f == 0:
        return k * np.log(m) - m - special.gammaln(k + 1)
    r = 1.0 / f
    return special.gammaln(r + k) - special.gammaln(r) - special.gammaln(k + 1) + k * np.log(m / (r + m)) + r * np.log(r / (r + m))


def exact_terms(x_a, x_b, s_a, s_b, mu, phi):
    T = int(x_a) + int(x_b)
    i = np.arange(T + 1, dtype=np.float64)
    # lp(T - i; ...) is the array of lp(k; ...), k ascending, read backwards: one evaluation per (k, parameters), so that with
    # s_a == s_b the term of i and the term of T - i are the same two numbers added
    return _lp(i, s_a * mu, phi / s_a) + _lp(i, s_b * mu, phi / s_b)[::-1]


def exact_p(x_a, x_b, s_a, s_b, mu, phi):
    l = exact_terms(x_a, x_b, s_a, s_b, mu, phi)
    w = np.exp(l - l.max())
    return float(np.sum(w[l <= l[int(x_a)]]) / np.sum(w))


def asymptotic_p(x_a, x_b, s_a, s_b, mu, phi):
    """-> (p, below the median)"""
    alpha = s_a * mu / (1 + phi * mu)
    beta = (s_b / s_a) * alpha
    T = float(x_a + x_b)
    med = stats.beta.median(alpha, beta)
    if (x_a + 0.5) / T < med:
        return 2 * float(special.betainc(alpha, beta, (x_a + 0.5) / T)), True, float(med)
    return 2 * float(special.betainc(beta, alpha, (x_b + 0.5) / T)), False, float(med)


def adjust_bh(p):
    p = np.asarray(p, dtype=np.float64)
    if len(p) == 0:
        return p.copy()
    descending = np.argsort(p)[::-1]
    scale = float(len(p)) / np.arange(len(p), 0, -1)
    q = np.minimum(1, np.minimum.accumulate(scale * p[descending]))
    return q[np.argsort(descending)]


def check_labels(labels, N, K):
    labels = np.asarray(labels)
    if K < 2 or len(labels) != N or labels.min() < 1 or labels.max() > K or len(np.unique(labels)) != K:
        raise ValueError("labels 1 .. K, every cluster with a cell, K >= 2")


def diffexp(x, params, labels, n_clusters, order=0, want_p=True):
    x = np.asarray(x)
    G, N = x.shape
    K = int(n_clusters)
    labels = np.asarray(labels)
    check_labels(labels, N, K)
    sf, use, mu, phi = params["size_factors"], params["use_g"], params["mean_g"], params["phi_g"]
    o = dict(sums_in=np.zeros((K, G), np.uint64), sums_out=np.zeros((K, G), np.uint64), norm_mean_in=np.zeros((K, G)), norm_mean_out=np.zeros((K, G)),
             log2_fold_change=np.zeros((K, G)), p_values=np.ones((K, G)), adjusted_p_values=np.ones((K, G)), below_median=np.full((K, G), 255, np.uint8),
             s_a=np.zeros(K), s_b=np.zeros(K), n_exact=np.zeros(K, np.uint64), n_asymptotic=np.zeros(K, np.uint64), median=np.full((K, G), np.nan),
             min_gap=np.full((K, G), np.inf))
    total = x.sum(axis=1).astype(np.uint64)
    for c in range(K):
        a = labels == c + 1
        s_a, s_b = float(_sum(sf[a], order)), float(_sum(sf[~a], order))
        x_a = x[:, a].sum(axis=1).astype(np.uint64)
        x_b = total - x_a
        o["s_a"][c], o["s_b"][c], o["sums_in"][c], o["sums_out"][c] = s_a, s_b, x_a, x_b
        o["norm_mean_in"][c], o["norm_mean_out"][c] = x_a / s_a, x_b / s_b
        o["log2_fold_change"][c] = np.log2((1 + x_a.astype(np.float64)) / (1 + s_a)) - np.log2((1 + x_b.astype(np.float64)) / (1 + s_b))
        if not want_p:
            continue
        for g in np.flatnonzero(use):
            xa, xb = int(x_a[g]), int(x_b[g])
            if xa > BIG_COUNT and xb > BIG_COUNT:
                p, left, med = asymptotic_p(xa, xb, s_a, s_b, mu[g], phi[g])
                o["p_values"][c, g], o["below_median"][c, g], o["median"][c, g] = p, 1 if left else 0, med
                o["n_asymptotic"][c] += 1
            else:
                l = exact_terms(xa, xb, s_a, s_b, mu[g], phi[g])
                w = np.exp(l - l.max())
                o["p_values"][c, g] = np.sum(w[l <= l[xa]]) / np.sum(w)
                gap = np.abs(l - l[xa])
                gap = gap[gap > 0]
                o["min_gap"][c, g] = gap.min() if len(gap) else np.inf
                o["n_exact"][c] += 1
        o["adjusted_p_values"][c, use] = adjust_bh(o["p_values"][c, use])
    o["data"] = np.zeros((G, 3 * K))
    o["data"][:, 0::3], o["data"][:, 1::3], o["data"][:, 2::3] = o["norm_mean_in"].T, o["log2_fold_change"].T, o["adjusted_p_values"].T
    return o


# ---- exact arithmetic ------------------------------------------------------------------------------------------------------------------
def _mp():
    import mpmath

    mpmath.mp.dps = 40
    return mpmath


def params_mp(x):
    """compute_params from the integers at 40 digits -> dict of lists of mpf (phi_g None for a gene that is not used)"""
    mp = _mp()
    x = np.asarray(x)
    G, N = x.shape
    counts = [int(v) for v in x.sum(axis=0)]
    srt = sorted(counts)
    med = mp.mpf(srt[N // 2]) if N % 2 else (mp.mpf(srt[N // 2 - 1]) + srt[N // 2]) / 2
    sf = [mp.mpf(c) / med for c in counts]
    S = mp.fsum(1 / s for s in sf)
    mean, var, use, phi_mm = [], [], [], []
    for g in range(G):
        xn = [int(x[g, c]) / sf[c] for c in range(N)]
        m = mp.fsum(xn) / N
        v = mp.fsum(t * t for t in xn) / N - m * m
        mean.append(m), var.append(v), use.append(v > mp.mpf(10) ** -30)
        phi_mm.append(max(mp.mpf(0), (N * v - m * S) / (m * m * S)) if use[-1] else mp.mpf(0))
    u = sorted(phi_mm[g] for g in range(G) if use[g])
    vi = (len(u) - 1) * mp.mpf(995) / 1000
    lo = int(mp.floor(vi))
    zeta = u[lo] + (u[min(lo + 1, len(u) - 1)] - u[lo]) * (vi - lo)
    any_pos = any(v > 0 for v in u)
    pm_mean = mp.fsum(u) / len(u)
    delta = (mp.fsum((v - pm_mean) ** 2 for v in u) / (G - 1)) / (mp.fsum((v - zeta) ** 2 for v in u) / (G - 2)) if any_pos else mp.nan
    phi = [((1 - delta) * phi_mm[g] + delta * zeta if any_pos else mp.mpf(0)) if use[g] else None for g in range(G)]
    return dict(size_factors=sf, mean_g=mean, var_g=var, use_g=use, phi_mm_g=phi_mm, phi_g=phi, zeta_hat=zeta, delta=delta)


def exact_p_mp(x_a, x_b, s_a, s_b, mu, phi):
    """the exact test at 40 digits: the terms by their ratios w_(i + 1) / w_i = (r_a + i) (T - i) / ((i + 1) (r_b + T - i - 1)); with phi == 0
    (s_a / s_b) (T - i) / (i + 1).  A term within 1e-30 (relative) of the observed one counts as equal to it (the mirrored term)."""
    mp = _mp()
    T = int(x_a) + int(x_b)
    s_a, s_b, phi = mp.mpf(s_a), mp.mpf(s_b), mp.mpf(phi)
    w = [mp.mpf(1)]
    if phi == 0:
        for i in range(T):
            w.append(w[-1] * (s_a / s_b) * (T - i) / (i + 1))
    else:
        ra, rb = s_a / phi, s_b / phi
        for i in range(T):
            w.append(w[-1] * (ra + i) * (T - i) / ((i + 1) * (rb + T - i - 1)))
    lim = w[int(x_a)] * (1 + mp.mpf(10) ** -30)
    return mp.fsum(v for v in w if v <= lim) / mp.fsum(w)


def asymptotic_p_mp(x_a, x_b, s_a, s_b, mu, phi):
    mp = _mp()
    s_a, s_b, mu, phi = mp.mpf(s_a), mp.mpf(s_b), mp.mpf(mu), mp.mpf(phi)
    alpha = s_a * mu / (1 + phi * mu)
    beta = (s_b / s_a) * alpha
    T = mp.mpf(int(x_a) + int(x_b))
    cdf = lambda a, b, v: mp.betainc(a, b, 0, v, regularized=True)
    lo, hi = mp.mpf(0), mp.mpf(1)
    for _ in range(70):
        mid = (lo + hi) / 2
        if cdf(alpha, beta, mid) < 0.5:
            lo = mid
        else:
            hi = mid
    med = (lo + hi) / 2
    if (int(x_a) + mp.mpf(1) / 2) / T < med:
        return 2 * cdf(alpha, beta, (int(x_a) + mp.mpf(1) / 2) / T), True, med
    return 2 * cdf(beta, alpha, (int(x_b) + mp.mpf(1) / 2) / T), False, med


def diffexp_mp(x, labels, n_clusters):
    """every p-value and adjusted p-value in exact arithmetic from the integer matrix -> (p f64[K, G], adjusted f64[K, G], medians)"""
    mp = _mp()
    x = np.asarray(x)
    G, N = x.shape
    K = int(n_clusters)
    labels = np.asarray(labels)
    P = params_mp(x)
    use = np.array(P["use_g"], bool)
    p, adj, med = np.ones((K, G)), np.ones((K, G)), np.full((K, G), np.nan)
    total = x.sum(axis=1)
    for c in range(K):
        a = labels == c + 1
        s_a = mp.fsum(P["size_factors"][i] for i in np.flatnonzero(a))
        s_b = mp.fsum(P["size_factors"][i] for i in np.flatnonzero(~a))
        x_a = x[:, a].sum(axis=1)
        pc = {}
        for g in np.flatnonzero(use):
            xa, xb = int(x_a[g]), int(total[g] - x_a[g])
            if xa > BIG_COUNT and xb > BIG_COUNT:
                v, _, m = asymptotic_p_mp(xa, xb, s_a, s_b, P["mean_g"][g], P["phi_g"][g])
                med[c, g] = float(m)
            else:
                v = exact_p_mp(xa, xb, s_a, s_b, P["mean_g"][g], P["phi_g"][g])
            pc[g] = v
        genes = sorted(pc, key=lambda g: pc[g])
        n, run = len(genes), None
        for k in range(n, 0, -1):
            v = pc[genes[k - 1]] * n / k
            run = v if run is None or v < run else run
            adj[c, genes[k - 1]] = float(min(run, mp.mpf(1)))
        for g in pc:
            p[c, g] = float(pc[g])
    return p, adj, med, P


# ---- fixtures ----------------------------------------------------------------------------------------------------------------------------
FIXTURES = {
    "base": dict(seed=101, G=60, N=257, K=3),
    "two_cells_one_cluster": dict(seed=102, G=12, N=2, K=2),
    "constant_rows": dict(seed=103, G=20, N=48, K=2),
    "poisson": dict(seed=104, G=16, N=40, K=2),
    "mirror": dict(seed=105, G=24, N=60, K=2),
    "long_tail": dict(seed=106, G=14, N=100, K=2),
    "k10": dict(seed=107, G=30, N=64, K=10),
    "g3": dict(seed=108, G=3, N=20, K=2),
}
CONSTRUCTED_900 = {"long_tail"}      # the fixtures whose count sums sit on the 900 boundary on purpose


def _labels(rs, N, K):
    lab = np.concatenate([np.arange(1, K + 1), rs.randint(1, K + 1, N - K)]) if N >= K else np.arange(1, N + 1)
    rs.shuffle(lab)
    return lab.astype(np.int32)


def _nb_matrix(rs, G, N, labels, K, top=25.0):
    """negative-binomial counts: gene means log-uniform up to `top`, a depth per cell, a cluster effect on a third of the genes"""
    base = np.exp(rs.uniform(np.log(0.05), np.log(top), G))
    depth = np.exp(rs.normal(0.0, 0.35, N))
    effect = np.ones((G, K))
    for g in range(G):
        if rs.rand() < 0.35:
            effect[g, rs.randint(K)] = np.exp(rs.normal(0.0, 1.0))
    mu = base[:, None] * depth[None, :] * effect[:, labels - 1]
    r = 1.0 / rs.uniform(0.05, 1.5, G)[:, None]
    x = rs.negative_binomial(r, r / (r + mu)).astype(np.int64)
    x[0, x.sum(axis=0) == 0] = 1      # no empty cell
    return x


def fixture(name, bump=0):
    """-> (x int64[G, N], labels i32[N], K)"""
    f = FIXTURES[name]
    G, N, K = f["G"], f["N"], f["K"]
    rs = np.random.RandomState(f["seed"] + 1000 * bump)
    if name == "two_cells_one_cluster":
        labels = np.array([1, 2], np.int32)
        return _nb_matrix(rs, G, N, labels, K, top=40.0) + 1, labels, K
    if name == "constant_rows":
        # column sums M 2^j make the size factors powers of two; row 1 is 4 x size factor, row 0 is empty, the last row fills the column
        labels = _labels(rs, N, K)
        x = _nb_matrix(rs, G, N, labels, K, top=8.0)
        j = np.array([0] * (N // 2 + 1) + [1] * (N // 4) + [-1] * (N - N // 2 - 1 - N // 4))
        rs.shuffle(j)
        x[0], x[1], x[2] = 0, (4 * 2.0 ** j).astype(np.int64), 0
        x[G - 1] = 0
        M = 1 << int(np.ceil(np.log2(x.sum(axis=0).max() * 2 + 2)))
        x[G - 1] = (M * 2.0 ** j).astype(np.int64) - x.sum(axis=0)
        return x, labels, K
    if name == "poisson":
        # rows in complementary pairs m + b, m' + (1 - b): equal column sums (every size factor 1), variance below the mean: phi_mm = 0
        labels = _labels(rs, N, K)
        x = np.zeros((G, N), np.int64)
        for p in range(G // 2):
            b = rs.randint(0, 2, N)
            if b.min() == b.max():
                b[0] = 1 - b[0]
            x[2 * p], x[2 * p + 1] = rs.randint(1, 60) + b, rs.randint(1, 60) + 1 - b
        return x, labels, K
    if name == "mirror":
        # the second half of the cells repeats the first with the genes swapped in pairs: equal size factors in equal order, s_a == s_b
        h = N // 2
        half = _nb_matrix(rs, G, h, np.ones(h, np.int32), 1, top=30.0)
        swap = np.arange(G).reshape(-1, 2)[:, ::-1].ravel()
        return np.concatenate([half, half[swap]], axis=1), np.repeat(np.array([1, 2], np.int32), h), K
    if name == "long_tail":
        na = 30
        labels = np.array([1] * na + [2] * (N - na), np.int32)
        x = _nb_matrix(rs, G, N, labels, K, top=6.0)

        def spread(total, n):
            return rs.multinomial(total, np.full(n, 1.0 / n))

        x[0, :na], x[0, na:] = spread(4, na), spread(70000, N - na)
        for k, (xa, xb) in enumerate(((899, 1003), (900, 1010), (901, 998), (1007, 899), (1012, 900), (995, 901))):
            x[1 + k, :na], x[1 + k, na:] = spread(xa, na), spread(xb, N - na)
        return x, labels, K
    labels = _labels(rs, N, K)
    return _nb_matrix(rs, G, N, labels, K, top=25.0 if name == "base" else 12.0), labels, K
