"""numpy restatement of the JIBES tag caller (CALL_TAGS_JIBES): the latent states, the prior, the EM fit and the assignments.

Restated from lib/rust/jibes_o3/src/lib.rs (what runs in production) and, for the parts the Rust calls back into Python for,
from cellranger.analysis.combinatorics, cellranger.feature.feature_assigner and cellranger.analysis.jibes.  Where the Rust and
jibes_py.py differ (strict stop comparisons, the slope clamp, the sd floor, the variance over elem_11) the Rust is followed.

The order of the additions that matters is kept: a state's log posterior is the prior plus the tags' log densities in tag order;
ln_pdf is statrs' (-0.5 d d) - ln sqrt(2 pi) - ln sd with d = (x - mu) / sd.  Cross-barcode sums are numpy's; the reference's own
are sequential (ndarray folds), which is one of the reorderings jibes_movement (tests/golden/jibes_reference.npz) measures.

_exp and _log are the two transcendental functions of the E step; the golden recorder swaps them for versions that move every
result by -1, 0 or +1 ulp to stand in for another math library."""
import math

import numpy as np

CORR_FACTOR = 1.54
N_G = 95000
G19_N_GEMS = {"MT": N_G, "LT": 9500, "HT": 190000}
NUM_TOTAL_TAGS = 14
MAX_K_LETS = 3
MIN_FOREGROUND_DELTA = 0.01
SD_FLOOR = 0.0001
LN_SQRT_2PI = 0.91893853320467274178      # statrs::consts::LN_SQRT_2PI
DEFAULT_BLANK = 0.04
JIBES_MIN_CONFIDENCE = 0.9
NEAR_ZERO_MAX = 12
OTHER = -1      # a preliminary call that is no single tag
BOUND_FACTOR = 16

_exp = np.exp
_log = np.log


# ---- latent states (combinatorics.py) --------------------------------------------------------------------------------------------
def generate_solutions(elements, k):
    if elements == 1:
        yield [k]
        return
    for i in range(k + 1):
        for val in generate_solutions(elements - 1, k - i):
            yield [i] + val


def generate_all_multiplets(n_tags, max_multiplets, add_unit_vector_at_end=False):
    out = []
    for k in range(max_multiplets + 1):
        out += list(generate_solutions(n_tags, k))
    if add_unit_vector_at_end:
        out.append([1] * n_tags)
    return np.array(out, dtype=np.int32)


# ---- Poisson loading (feature_assigner.py) -----------------------------------------------------------------------------------------
def multiplet_counts_unrounded(obs_cells, n_gems=N_G, n_entries=NUM_TOTAL_TAGS):
    """get_multiplet_counts_unrounded: expected GEMs with 1 .. 14 cells; the pmf is exp(k ln mu - lgamma(k + 1) - mu)"""
    mu = float(CORR_FACTOR * obs_cells) / n_gems
    if mu <= 0.0:
        return np.zeros(n_entries)
    pmf = np.array([math.exp(j * math.log(mu) - math.lgamma(j + 1.0) - mu) for j in range(1, n_entries + 1)])
    return pmf * n_gems / CORR_FACTOR


LAMBDA_PEAK = math.exp(math.lgamma(15.0) / 14.0)      # d/d mu P(1 <= J <= 14) = pmf(0) - pmf(14) = 0  <=>  mu^14 = 14!


class CellEstimateCantConverge(Exception):
    pass


def expected_total_cells(obs_barcodes, n_gems=N_G):
    """The root x of sum(multiplet_counts_unrounded(x)) = obs_barcodes by bisection on the rising branch [0, LAMBDA_PEAK n_gems / 1.54].
    The reference minimises the squared difference with BFGS from 1.1 n and keeps where that stops; it raises when the minimum
    is above 2, i.e. when |difference| > sqrt(2): so does this."""
    def f(x):
        return float(np.sum(multiplet_counts_unrounded(x, n_gems))) - obs_barcodes

    lo, hi = 0.0, LAMBDA_PEAK * n_gems / CORR_FACTOR
    if obs_barcodes <= 0:
        return 0.0
    if f(hi) < 0.0:
        if f(hi) * f(hi) > 2.0:
            raise CellEstimateCantConverge("Could not converge on an accurate cell estimate.")
        return hi
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if mid <= lo or mid >= hi:
            break
        if f(mid) < 0.0:
            lo = mid
        else:
            hi = mid
    return hi


def latent_state_setup(n, k, n_gems, max_k_lets=MAX_K_LETS, estimated_cells=None):
    """JibesEMO3::new: (states, k_let_limited, max_multiplets, max_modeled_k_let, estimated_cells)"""
    if estimated_cells is None:
        estimated_cells = expected_total_cells(n, n_gems)
    exp_cnts = np.round(multiplet_counts_unrounded(estimated_cells, n_gems))
    nz = np.nonzero(exp_cnts > 0.0)[0]
    max_multiplets = max(int(nz.max()) + 1, 2) if len(nz) else 4
    limited = False
    if max_multiplets > max_k_lets:
        limited, max_multiplets = True, max_k_lets
    states = generate_all_multiplets(k, max_multiplets, limited)
    return states, limited, max_multiplets, max(k, max_multiplets), estimated_cells


def _lfactorial(x):
    return math.log(float(math.factorial(int(x))))      # statrs ln_factorial: ln of the cached factorial


def log_prior(states, estimated_cells, n_gems, limited, max_modeled_k_let, max_k_lets=MAX_K_LETS, blank=DEFAULT_BLANK, freqs=None):
    """calculate_latent_state_weights of the Rust.  QUIRK kept: with k <= max_k_lets and a limited model the overwritten last entry
    of p_k_let is an empty sum; the states that index it get -inf.
    Beyond the reference: it has 14 Poisson counts, so with 15 or 16 tags and a limited model its unit-vector state indexes past
    them (an index error there).  Here the counts run to max(14, k); for k <= 14 nothing changes."""
    z, k = states.shape
    freqs = np.full(k, 1.0 / k) if freqs is None else np.asarray(freqs, np.float64)
    cnts = multiplet_counts_unrounded(estimated_cells, n_gems, max(NUM_TOTAL_TAGS, k))[:max_modeled_k_let]
    p_k_let = cnts / np.sum(cnts)
    if limited:
        p_k_let[-1] = np.sum(p_k_let[max_k_lets:])
    klet = states.sum(axis=1)
    pis = [math.log(f) for f in freqs]
    out = np.zeros(z)
    out[0] = math.log(blank)
    log_not_blank = math.log(1.0 - blank)
    for zi in range(1, z):
        rel = [i for i in range(k) if states[zi, i] != 0]
        c = [float(states[zi, i]) for i in rel]
        mult = _lfactorial(sum(c)) - sum(_lfactorial(v) for v in c)
        p = 0.0
        for cnt, i in zip(c, rel):
            p += cnt * pis[i]
        pk = p_k_let[klet[zi] - 1]
        out[zi] = p + mult + (math.log(pk) if pk > 0.0 else -math.inf) + log_not_blank
    return out


# ---- the fit ---------------------------------------------------------------------------------------------------------------------------
def e_step(Y, states, prior, bg, fg, sd):
    """_calculate_posterior_by_state: (posterior, LL)"""
    n, k = Y.shape
    X = states.astype(np.float64)
    P = np.tile(prior, (n, 1))
    for t in range(k):
        mu = bg[t] + fg[t] * X[:, t]
        d = (Y[:, t][:, None] - mu[None, :]) / sd[t]
        P += (-0.5 * d * d) - LN_SQRT_2PI - float(_log(np.float64(sd[t])))
    mx = P.max(axis=1)
    P = _exp(P - mx[:, None])
    marg = P.sum(axis=1)
    P /= marg[:, None]
    return P, float(_log(marg).sum() + mx.sum())


def m_step(Y, states, P):
    """maximize_parameters: the closed-form 2 x 2 weighted least squares per tag -> (bg, fg, sd)"""
    n, k = Y.shape
    X = states.astype(np.float64)
    bg, fg, sd = np.zeros(k), np.zeros(k), np.zeros(k)
    e11 = P.sum()
    rows = P.sum(axis=1)
    for t in range(k):
        px = (P * X[:, t][None, :]).sum(axis=1)
        first = (Y[:, t] * rows).sum()
        second = (Y[:, t] * px).sum()
        e12 = px.sum()
        e22 = ((P * X[:, t][None, :]) * X[:, t][None, :]).sum()
        det = 1.0 / (e11 * e22 - e12 * e12)
        c0 = (det * e22) * first + (det * -e12) * second
        c1 = (det * -e12) * first + (det * e11) * second
        if c1 < MIN_FOREGROUND_DELTA:
            c1 = MIN_FOREGROUND_DELTA
            c0 = first / e11 - MIN_FOREGROUND_DELTA * (e12 / e11)
        r = (c1 * X[:, t] + c0)[None, :] - Y[:, t][:, None]
        res = (r * r * P).sum()
        bg[t], fg[t], sd[t] = c0, c1, max(math.sqrt(res / e11), SD_FLOOR)
    return bg, fg, sd


def perform_em(Y, states, prior, bg, fg, sd, max_reps=50000, abs_tol=1e-2, rel_tol=1e-7):
    """perform_EM of the Rust -> dict(iterations, converged, LL, lls (LL after every E step, the initial one first), bg, fg, sd, posterior)"""
    Y = np.asarray(Y, np.float64)
    bg, fg, sd = (np.array(a, np.float64) for a in (bg, fg, sd))
    n, k = Y.shape
    if n == 0:
        return dict(iterations=0, converged=True, LL=0.0, lls=np.zeros(0), bg=bg, fg=np.zeros(k), sd=sd, posterior=np.zeros((0, len(states))))
    assert np.all(fg >= MIN_FOREGROUND_DELTA)
    P, LL = e_step(Y, states, prior, bg, fg, sd)
    lls, last, rep, converged = [LL], -math.inf, 0, False
    while True:
        bg, fg, sd = m_step(Y, states, P)
        P, LL = e_step(Y, states, prior, bg, fg, sd)
        rep += 1
        lls.append(LL)
        if rep > max_reps:
            break
        if last != -math.inf and ((LL - last < abs_tol) or (1.0 - LL / last < rel_tol)):
            converged = True
            break
        last = LL
    return dict(iterations=rep, converged=converged, LL=LL, lls=np.array(lls), bg=bg, fg=fg, sd=sd, posterior=P)


# ---- assignments (jibes.get_assignment_df, JibesTagAssigner.get_tag_assignments) ----------------------------------------------------------
def state_classes(states):
    """get_cols_associated_with_assignments: per state 0 .. k - 1 = only that tag (any multiplicity), k = Multiplet, k + 1 = Blank.
    A state that is not blank holds only tag t for at most one t, so the classes do not overlap."""
    z, k = states.shape
    rs = states.sum(axis=1)
    cls = np.full(z, k, np.int32)
    for t in range(k):
        cls[(states[:, t] == rs) & (rs > 0)] = t
    cls[rs == 0] = k + 1
    return cls


def assignment_table(posterior, states, confidence=JIBES_MIN_CONFIDENCE, exclude_blanks=False, apply_confidence=True):
    """-> dict(probs n x (k + 2) in the order tags, Multiplet, Blank; candidate; assignment (k + 2 = Unassigned); probability;
    ml_state = the most likely multiplet STATE INDEX (first maximum over the multiplet columns, ascending))"""
    z, k = states.shape
    n = posterior.shape[0]
    cls = state_classes(states)
    probs = np.zeros((n, k + 2))
    for c in range(k + 2):
        idx = np.nonzero(cls == c)[0]
        probs[:, c] = posterior[:, idx].sum(axis=1) if len(idx) else 0.0
    cand = probs.argmax(axis=1).astype(np.int32) if n else np.zeros(0, np.int32)
    prob = probs.max(axis=1) if n else np.zeros(0)
    asst = cand.copy()
    if apply_confidence:
        p = prob.copy()
        if exclude_blanks:
            nb = cand != k + 1
            p[nb] = p[nb] / (1.0 - probs[nb, k + 1])
        asst[p < confidence] = k + 2
    midx = np.nonzero(cls == k)[0]
    ml = midx[posterior[:, midx].argmax(axis=1)].astype(np.int32) if (n and len(midx)) else np.zeros(n, np.int32)
    return dict(probs=probs, candidate=cand, assignment=asst, probability=prob, ml_state=ml)


def tag_assignments(table, states, kept, near_zero):
    """get_tag_assignments: kept / near_zero = the barcode indices (of the filtered matrix) that entered the fit / were set aside.
    -> (barcodes per tag, dict Blank / Unassigned / Multiplet)"""
    z, k = states.shape
    per_tag = [[] for _ in range(k)]
    non = {"Blank": [], "Unassigned": [], "Multiplet": []}
    for i, bc in enumerate(kept):
        a = int(table["assignment"][i])
        if a < k:
            per_tag[a].append(int(bc))
        elif a == k:
            non["Multiplet"].append(int(bc))
            for t in range(k):
                if states[table["ml_state"][i], t] > 0:
                    per_tag[t].append(int(bc))
        else:
            non["Blank" if a == k + 1 else "Unassigned"].append(int(bc))
    non["Blank"] += [int(b) for b in near_zero]
    return per_tag, non


def tag_table(dense_counts, valid):
    """JibesTagAssigner.__init__: dense_counts n x k_all integers, valid = mask of the tags kept.  The near-zero rule is over ALL tags.
    -> (row sums, near-zero indices, kept indices, log10(count + 1) of the kept barcodes and valid tags)"""
    dense = np.asarray(dense_counts, np.float64)
    row_sums = dense.sum(axis=1)
    nz = row_sums <= NEAR_ZERO_MAX
    logs = np.log10(dense + 1.0)[:, np.asarray(valid, bool)]
    return row_sums, np.nonzero(nz)[0], np.nonzero(~nz)[0], logs[~nz]


# ---- initial parameters (jibes.create_initial_parameters) ------------------------------------------------------------------------------------
def initial_parameters(Y, calls):
    """calls: per barcode a tag index or OTHER -> (bg, fg, sd)"""
    Y = np.asarray(Y, np.float64)
    calls = np.asarray(calls)
    k = Y.shape[1]
    fg, sd, bg = np.zeros(k), np.zeros(k), np.zeros(k)
    bad = []
    singletons = (calls >= 0) & (calls < k)
    for i in range(k):
        vals = calls == i
        if np.sum(vals) < 2:
            fg[i] = bg[i] = sd[i] = np.nan
            bad.append(i)
            continue
        other = (calls != i) & singletons
        bg[i] = Y[other, i].mean() if np.sum(other) > 0 else Y[:, i].mean()
        f = Y[vals, i]
        fg[i] = np.maximum(0.6 + bg[i], np.mean(f)) - bg[i]
        sd[i] = f.std()
    if bad:
        if len(bad) == k:
            fg[bad], bg[bad], sd[bad] = 1.0, 0.5, 0.3
        else:
            good = [x for x in range(k) if x not in bad]
            fg[bad], bg[bad], sd[bad] = np.mean(fg[good]), np.mean(bg[good]), np.mean(sd[good])
    sd[sd == 0.0] = 0.2
    return bg, fg, sd


# ---- the stage -----------------------------------------------------------------------------------------------------------------------------
def call_tags(dense_counts, valid, prelim_calls, n_gems, confidence=JIBES_MIN_CONFIDENCE, exclude_blanks=False, estimated_cells=None,
              abs_tol=0.1, rel_tol=1e-7, max_reps=50000):
    """run_assignment_stage + get_tag_assignments on the dense tag counts of the filtered matrix.  prelim_calls: per barcode of the
    matrix an index into the VALID tags or OTHER."""
    row_sums, near_zero, kept, Y = tag_table(dense_counts, valid)
    k = Y.shape[1]
    bg, fg, sd = initial_parameters(Y, np.asarray(prelim_calls)[kept])
    states, limited, _, mmk, est = latent_state_setup(len(kept), k, n_gems, estimated_cells=estimated_cells)
    prior = log_prior(states, est, n_gems, limited, mmk)
    fit = perform_em(Y, states, prior, bg, fg, sd, max_reps=max_reps, abs_tol=abs_tol, rel_tol=rel_tol)
    table = assignment_table(fit["posterior"], states, confidence, exclude_blanks)
    per_tag, non = tag_assignments(table, states, kept, near_zero)
    return dict(fit=fit, table=table, per_tag=per_tag, non_singlets=non, snr=fit["fg"] / fit["sd"], states=states, kept=kept, near_zero=near_zero)
