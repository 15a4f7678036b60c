"""numpy restatement of the multi-genome analysis (lib/python/cellranger/analysis/multigenome.py:80-335), written from its
contract: classify (classify_gems, :138-177), bootstrap (_infer_multiplets, :209-249, with the real np.random.seed(0) /
np.random.choice), infer (infer_multiplets_from_observed, :113-135), summary (:287-301), purity (the mean purities of
compute_count_purity, :80-98) and top_two (:256-262).  What the device path must equal, number for number.

Calls: 0 genome0, 1 genome1, 2 Multiplet.  Branch codes: 0 default thresholds, 1 per-genome percentiles, +2 when the
fold-change test replaced both by the percentile of c0 + c1 (2 itself cannot occur: 10 / 10 never passes the test)."""
import numpy as np

GENOME0, GENOME1, MULTIPLET = 0, 1, 2
DEFAULT_THRESHOLD = 10
PROB_THRESHOLD = 0.1


def classify(c0, c1):
    """-> (call int8[n], t0, t1, branch); thresholds as python / numpy floats"""
    c0, c1 = np.asarray(c0, np.int64), np.asarray(c1, np.int64)
    t0 = t1 = DEFAULT_THRESHOLD
    branch = 0
    if (c0 > c1).sum() >= 1 and (c1 > c0).sum() >= 1:
        t0 = np.percentile(c0[c0 > c1], PROB_THRESHOLD * 100.0)
        t1 = np.percentile(c1[c1 > c0], PROB_THRESHOLD * 100.0)
        branch = 1
    lo, hi = sorted([t0, t1])
    with np.errstate(divide="ignore", invalid="ignore"):
        fold = np.float64(hi) / np.float64(lo)
    if lo < 50 and fold > 25:
        t0 = t1 = np.percentile(c0 + c1, PROB_THRESHOLD * 100.0)
        branch += 2
    call = np.where(np.logical_and(c0 >= t0, c1 >= t1), MULTIPLET, GENOME0).astype(np.int8)
    call[np.logical_and(call != MULTIPLET, c1 > c0)] = GENOME1
    return call, float(t0), float(t1), branch


def infer(m, g0, g1):
    if g0 == 0 or g1 == 0:
        return 0
    p = 2 * (float(g0) / float(g0 + g1)) * (float(g1) / float(g0 + g1))
    return min(float(m) / p, float(m + g0 + g1))


def bootstrap(c0, c1, bootstraps=1000):
    """-> (boot_counts int64[B, 3] = (Multiplets, genome0, genome1), thresholds float64[B, 2], branch int32[B])"""
    c0, c1 = np.asarray(c0, np.int64), np.asarray(c1, np.int64)
    n = len(c0)
    counts, thr, br = np.zeros((bootstraps, 3), np.int64), np.zeros((bootstraps, 2), np.float64), np.zeros(bootstraps, np.int32)
    np.random.seed(0)
    for s in range(bootstraps):
        idx = np.random.choice(n, n)
        call, t0, t1, b = classify(c0[idx], c1[idx])
        counts[s] = [(call == MULTIPLET).sum(), (call == GENOME0).sum(), (call == GENOME1).sum()]
        thr[s] = [t0, t1]
        br[s] = b
    return counts, thr, br


def _robust_divide(a, b):
    a, b = float(a), float(b)
    return float("nan") if b == 0 else a / b


def summary(boot_counts, n):
    """the numbers of :287-301 from the per-sample class counts -> dict (boot: float64[B])"""
    boot = np.zeros(len(boot_counts))
    for s, (m, g0, g1) in enumerate(np.asarray(boot_counts, np.int64).tolist()):
        boot[s] = infer(m, g0, g1)
    rate = _robust_divide(boot.mean(), n)
    out = dict(boot=boot, mean=float(boot.mean()), inferred_multiplets=int(round(boot.mean())), rate=rate,
               normalized_rate=1000 * _robust_divide(rate, n), rate_lb=None, rate_ub=None)
    if boot.size > 1:
        out["rate_lb"] = _robust_divide(np.percentile(boot, 2.5), n)
        out["rate_ub"] = _robust_divide(np.percentile(boot, 97.5), n)
    return out


def purity(c0, c1, call):
    """-> (six integer sums, (purity0, purity1, overall))"""
    c0, c1, call = np.asarray(c0, np.int64), np.asarray(c1, np.int64), np.asarray(call)
    g0, g1 = call == GENOME0, call == GENOME1
    single = g0 | g1
    sums = (int(c0[g0].sum()), int((c0[g0] + c1[g0]).sum()), int(c1[g1].sum()), int((c0[g1] + c1[g1]).sum()),
            int(np.maximum(c0[single], c1[single]).sum()), int((c0 + c1)[single].sum()))
    return sums, (_robust_divide(sums[0], sums[1]), _robust_divide(sums[2], sums[3]), _robust_divide(sums[4], sums[5]))


def top_two(totals):
    """sorted(argsort(totals)[::-1][:2]) with a stable argsort: among equal totals the larger index first"""
    return sorted(np.argsort(np.asarray(totals), kind="stable")[::-1][:2].tolist())


def run(c0, c1, bootstraps=1000):
    """everything the device call reports -> dict"""
    call, t0, t1, branch = classify(c0, c1)
    counts, thr, br = bootstrap(c0, c1, bootstraps)
    sums, pur = purity(c0, c1, call)
    out = dict(call=call.astype(np.uint8), obs_thresh=(t0, t1), obs_branch=branch, boot_counts=counts, boot_thresholds=thr,
               boot_branch=br, observed=(int((call == MULTIPLET).sum()), int((call == GENOME0).sum()), int((call == GENOME1).sum())),
               purity_sums=sums, purity=pur, n=len(call))
    out.update(summary(counts, len(call)))
    return out


def mixture(n, seed, pure=False):
    """(c0, c1) int64[n] of a seeded species-mixing well: 60 % genome0 cells, 35 % genome1 cells, 5 % doublets (log-normal
    totals of a few thousand UMIs) over a background of 0 .. 59 counts of the other genome, in random order.  pure: a
    single-species well (c1 in 0 .. 2 everywhere), where the fold-change test sends classify to the sums."""
    rng = np.random.RandomState(seed)
    kind = rng.rand(n)
    big0 = np.round(rng.lognormal(8.0, 0.5, n)).astype(np.int64) + 200
    big1 = np.round(rng.lognormal(7.6, 0.5, n)).astype(np.int64) + 200
    bg0, bg1 = rng.randint(0, 60, n).astype(np.int64), rng.randint(0, 60, n).astype(np.int64)
    if pure:
        return np.where(kind < 0.9, big0, bg0), rng.randint(0, 3, n).astype(np.int64)
    is0, dbl = kind < 0.60, kind >= 0.95
    return np.where(is0 | dbl, big0, bg0), np.where(~is0, big1, bg1)
