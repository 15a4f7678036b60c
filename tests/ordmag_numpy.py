"""numpy restatement of the initial cell call (the expected values of tests/test_gpu_cell_calling.py and the CPU yardstick of
scripts/bench_cell_calling.py), written from the behaviour of lib/python/cellranger/cell_calling_helpers.py:832-964:
the order-of-magnitude filter with its bootstrap, the estimate of the recovered cells, the summary with its tie extension,
and the fixed cutoff.  One GEM group."""
import numpy as np

N_SAMPLES = 100          # bootstrap samples per phase
QUANTILE = 0.99          # the baseline barcode sits at the (1 - QUANTILE) * recovered_cells-th place from the top
MIN_RECOVERED = 50
MAX_TIE_EXTENSION = 0.20


def candidates(max_expected_cells):
    grid = np.linspace(1, np.log2(max_expected_cells), 2000)
    return np.unique(np.round(np.power(2, grid)).astype(int))


def within_ordmag(sample, baseline_idx):
    """how many values of the sample reach a tenth (rounded half to even, at least 1) of its (baseline_idx + 1)-th largest;
    baseline_idx may be an array: one answer per entry"""
    falling = -np.sort(-sample)                      # largest first
    tenth = np.round(0.1 * falling[baseline_idx])
    floor_ = np.maximum(1, tenth).astype(int)
    return np.searchsorted(-falling, -floor_, side="right")    # values >= floor_


def estimate_one(sample, max_expected_cells):
    """the grid value whose own order-of-magnitude count comes closest to it, and that distance"""
    grid = candidates(max_expected_cells)
    places = np.minimum(np.round(grid * (1 - QUANTILE)).astype(int), len(sample) - 1)
    miss = within_ordmag(sample, places) - grid
    loss = np.power(miss, 2) / grid
    best = int(np.argmin(loss))          # the first minimum
    return grid[best], loss[best]


def summarize(top_n_boot, nz, out):
    from scipy import stats

    mean, var = np.mean(top_n_boot), np.var(top_n_boot)
    sd = np.sqrt(var)
    out.update(mean=mean, var=var, cv=(sd / mean if mean != 0 else 0.0))
    with np.errstate(invalid="ignore"):
        out["lb_raw"], out["ub_raw"] = stats.norm.ppf(0.025, mean, sd), stats.norm.ppf(0.975, mean, sd)
    out["lb"], out["ub"] = np.round(out["lb_raw"], 0), np.round(out["ub_raw"], 0)
    nbcs = int(np.round(mean))
    out["filtered_bcs"], out["cutoff"], out["nbcs"], out["gave_up"] = nbcs, None, nbcs, False
    if nbcs > 0:
        # grow the call over barcodes that tie with the last one taken, one place at a time; once more than a fifth has been
        # added, stop and keep what the earlier steps wrote
        falling = -np.sort(-nz, kind="stable")
        last_taken = falling[nbcs - 1]
        for place in range(nbcs, len(falling)):
            if falling[place - 1] != last_taken:
                break
            if place + 1 - nbcs > MAX_TIE_EXTENSION * nbcs:
                out["gave_up"] = True
                break
            out["filtered_bcs"], out["cutoff"] = place + 1, int(last_taken)


def top_columns(bc_counts, top_n):
    """stable ascending argsort, reversed, first top_n, ascending: among equal counts the larger column wins"""
    return np.sort(np.argsort(bc_counts, kind="stable")[::-1][:top_n])


def ordmag(bc_counts, recovered_cells=None, max_expected_cells=1 << 18, choice_log=None):
    """-> (called columns, dict of everything the device result reports)"""
    bc_counts = np.asarray(bc_counts).astype(np.int64)
    rs = np.random.RandomState(0)
    nz = bc_counts[bc_counts > 0]
    out = dict(n_nonzero=len(nz), recovered_cells=0, recovered_boot=np.zeros(N_SAMPLES, np.int64), loss_boot=np.zeros(N_SAMPLES),
               baseline_bc_idx=0, top_n_boot=np.zeros(N_SAMPLES, np.int64), mean=0.0, var=0.0, cv=0.0, lb=0.0, ub=0.0,
               lb_raw=0.0, ub_raw=0.0, filtered_bcs=0, cutoff=None, estimated=False)
    if len(nz) == 0:
        return np.zeros(0, np.int64), out
    if recovered_cells is None:
        est = np.array([estimate_one(rs.choice(nz, len(nz)), max_expected_cells) for _ in range(N_SAMPLES)])
        out["recovered_boot"], out["loss_boot"], out["estimated"] = est[:, 0].astype(np.int64), est[:, 1], True
        recovered_cells = int(np.round(np.mean(est, axis=0)[0]))
    recovered_cells = max(recovered_cells, MIN_RECOVERED)
    out["recovered_cells"] = recovered_cells
    b = min(int(np.round(float(recovered_cells) * (1 - QUANTILE))), len(nz) - 1)
    out["baseline_bc_idx"] = b
    out["top_n_boot"] = np.array([within_ordmag(rs.choice(nz, len(nz)), b) for _ in range(N_SAMPLES)], dtype=np.int64)
    summarize(out["top_n_boot"], nz, out)
    return top_columns(bc_counts, out["filtered_bcs"]), out


def fixed_cutoff(bc_counts, force_cells):
    bc_counts = np.asarray(bc_counts).astype(np.int64)
    n = int((bc_counts > 0).sum())
    top_n = min(force_cells, n)
    desc = np.sort(bc_counts)[::-1]
    out = dict(n_nonzero=n, filtered_bcs=top_n, mean=float(top_n), var=0.0, cv=0.0, lb=float(top_n), ub=float(top_n),
               cutoff=int(desc[top_n]) if top_n < len(desc) else None)
    return top_columns(bc_counts, top_n), out
