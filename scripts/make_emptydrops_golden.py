#!/usr/bin/env python
"""Record the reference's own outputs of the EmptyDrops step for one fixture well -> tests/golden/emptydrops_reference.npz.

    python scripts/make_emptydrops_golden.py <reference checkout>/lib/python

Needs the reference's Python package on the given path (cellranger.stats and cellranger.sgt are imported from it; nothing of it
is copied), so it runs only where that checkout exists; the tests read the recorded file.  cellranger.cell_calling itself needs
numexpr and is not imported: the glue between the recorded functions (ambient set, profile assembly, BH) is
tests/emptydrops_numpy.py, which tests/test_emptydrops_restatement.py then pins against what is recorded here.

The fixture is tests/emptydrops_numpy.make_well(seed) with the three largest cells left out of the initial call, so that the
candidates' totals make steps of 1, of 2 - 19, of 20 - 999 and of >= 1000: every branch of the reference's simulation loop
(stats.py:143-197) is recorded.  The first seed is taken for which
  * at most 5 % of the candidates have a reference adjusted p-value inside [fdr / 2, 2 * fdr], and none lies between a factor
    of 2 and a factor of 4 from fdr,
  * no simulated value of the small table lies within 1e-9 (relative) of the observed value it is compared with.
Recorded: the inputs of every reference function called (so that a reader can re-run them), sgt_proportions,
eval_multinomial_loglikelihoods, compute_ambient_pvalues over NUM_SIMS simulations of simulate_multinomial_loglikelihoods, and
one small table (12 distinct N x 500 simulations) with its p-values for the equality tests."""
import os
import sys

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import emptydrops_numpy as R  # noqa: E402

NUM_SIMS, TABLE_SIMS, TABLE_ROWS, DROPPED_CELLS = 1000, 500, 12, 3
OUT = os.path.join(ROOT, "tests", "golden", "emptydrops_reference.npz")


def fixture(seed):
    indptr, indices, data, nf, kind = R.make_well(seed)
    umis = R.column_sums(indptr, indices, data, nf)
    cells = np.flatnonzero(kind == 0)
    cells = np.sort(cells[np.argsort(umis[cells], kind="stable")[:-DROPPED_CELLS]])
    return indptr, indices, data, nf, kind, umis, cells


def main(ref_path):
    sys.path.insert(0, ref_path)
    import cellranger.sgt as cr_sgt
    import cellranger.stats as cr_stats

    F = R.FIXTURE
    for seed in range(1, 50):
        indptr, indices, data, nf, kind, umis_per_bc, cells = fixture(seed)
        use_bcs, max_bg = R.ambient_set(umis_per_bc, F["low"], F["high"])
        eval_features = np.flatnonzero(R.row_sums(indptr, indices, data, nf))
        profile = R.row_sums(indptr, indices, data, nf, use_bcs)[eval_features]
        seen = np.flatnonzero(profile)
        freq = profile[seen]
        pstar, p0 = cr_sgt.sgt_proportions(freq)
        n0 = len(profile) - len(seen)
        profile_p = np.repeat(p0 / n0 if n0 else -1.0, len(profile))
        profile_p[seen] = pstar if n0 else pstar / pstar.sum()
        thr = max(F["minimum_umis"], 1 + max_bg)
        cand = umis_per_bc >= thr
        cand[cells] = False
        eval_cols = np.flatnonzero(cand)
        umis = umis_per_bc[eval_cols]
        step = np.diff(np.flatnonzero(np.bincount(umis)))
        if not ((step == 1).any() and ((step >= 2) & (step < 20)).any() and ((step >= 20) & (step < 1000)).any() and (step >= 1000).any()):
            continue
        m = sp.csc_matrix((data, indices, indptr), shape=(nf, len(umis_per_bc)))
        eval_mat = m[eval_features, :][:, eval_cols]
        obs = cr_stats.eval_multinomial_loglikelihoods(eval_mat, profile_p)
        sim_n, sim_loglk = cr_stats.simulate_multinomial_loglikelihoods(profile_p, umis, num_sims=NUM_SIMS)
        pvalues = cr_stats.compute_ambient_pvalues(umis, obs, sim_n, sim_loglk)
        adj = R.adjust_pvalue_bh(pvalues)
        band = np.sum((adj >= F["fdr"] / 2) & (adj <= 2 * F["fdr"]))
        if band > 0.05 * len(umis):
            continue
        # A p-value near fdr rests on ~10 of NUM_SIMS simulations: another random stream moves it by a factor of 2 at about 1.5
        # standard deviations.  A candidate just outside the band would make the calls of two correct simulations differ, so
        # the fixture has none between a factor of 2 and a factor of 4 from fdr (decided on the reference's values alone; a
        # candidate below every simulation, p = 1 / (1 + NUM_SIMS), is not such a borderline case).
        ring = ((adj >= F["fdr"] / 4) & (adj < F["fdr"] / 2)) | ((adj > 2 * F["fdr"]) & (adj <= 4 * F["fdr"]))
        if np.any(ring & (pvalues > 1.0 / (1 + NUM_SIMS))):
            continue
        # the small table: candidates at TABLE_ROWS distinct N that span all step classes (the smallest totals, where steps of 1
        # and of 2 - 19 lie, and the dropped cells)
        dn = np.flatnonzero(np.bincount(umis))
        rows_n = np.concatenate((dn[: TABLE_ROWS - DROPPED_CELLS - 1], dn[-(DROPPED_CELLS + 1):]))
        tab_cand = np.flatnonzero(np.isin(umis, rows_n))
        tab_n, tab_loglk = cr_stats.simulate_multinomial_loglikelihoods(profile_p, umis[tab_cand], num_sims=TABLE_SIMS)
        assert np.array_equal(tab_n, rows_n)
        tstep = np.diff(tab_n)
        assert (tstep == 1).any() and ((tstep >= 2) & (tstep < 20)).any() and ((tstep >= 20) & (tstep < 1000)).any() and (tstep >= 1000).any()
        if R.near_tie(obs[tab_cand], umis[tab_cand], tab_n, tab_loglk):
            continue
        tab_p = cr_stats.compute_ambient_pvalues(umis[tab_cand], obs[tab_cand], tab_n, tab_loglk)
        tab_adj = R.adjust_pvalue_bh(tab_p)
        break
    else:
        raise SystemExit("no seed met the conditions")
    cand_csc = m[:, eval_cols]
    assert cand_csc.indices.max() < 65536 and cand_csc.data.max() < 2 ** 31
    np.savez_compressed(
        OUT, well_seed=seed, dropped_cells=DROPPED_CELLS, num_sims=NUM_SIMS, low=F["low"], high=F["high"], minimum_umis=F["minimum_umis"],
        fdr=F["fdr"], cell_cols=cells.astype(np.int32), n_ambient_used=len(use_bcs), max_background_umis=max_bg,
        eval_features=eval_features.astype(np.int32), profile=profile.astype(np.int64), eval_cols=eval_cols.astype(np.int32),
        umis=umis.astype(np.int64), cand_indptr=cand_csc.indptr.astype(np.int32), cand_indices=cand_csc.indices.astype(np.uint16),
        cand_data=cand_csc.data.astype(np.int32),
        ref_pstar=pstar, ref_p0=p0, ref_profile_p=profile_p, ref_obs_loglk=obs, ref_sim_n=sim_n.astype(np.int64), ref_pvalues=pvalues,
        ref_pvalues_adj=adj, tab_cand=tab_cand.astype(np.int32), tab_n=tab_n.astype(np.int64), tab_loglk=tab_loglk, tab_pvalues=tab_p,
        tab_pvalues_adj=tab_adj)
    size = os.path.getsize(OUT)
    print("seed %d: %d candidates, %d distinct N, %d in the band, %d bytes -> %s" % (seed, len(umis), len(sim_n), band, size, OUT))
    assert size < 256 * 1024


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
