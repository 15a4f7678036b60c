"""Time of the EmptyDrops step on the device (Context.call_additional_cells) and of its simulation kernel alone.
usage (GPU box): python3 scripts/bench_emptydrops.py [--features 36601] [--candidates 100000] [--sims 10000] [--repeats 3] [--no-cpu]

1. simulation   k_ed_simulate on a production-shaped problem: a log-normal profile over --features features, --candidates
                candidate totals (log-uniform 500 .. 20 000), --sims simulations; every candidate's observed value is the median
                of a 32-simulation pilot, so about half of the comparisons bump a counter.  Kernel milliseconds (HIP events)
                and draws per second (sims x largest total / time).  Variants that move one resource at a time:
                  one_n        all candidates at the largest total: one segment, no barrier per distinct N
                  few_features 64 features: the cdf and the guide table stay in the first cache levels, one counter takes many lanes
                  global       CRGPU_ED_LDS_FEATURES=0: the counters in global memory instead of LDS
2. whole step   call_additional_cells on a planted well (tests/emptydrops_numpy.make_well, 2 000 features, 45 000 columns):
                host milliseconds per call around a call that returns after the device has finished, and the kernel's share.
3. CPU          the numpy restatement of the same simulation (tests/emptydrops_numpy.simulate_philox) and the reference's
                scipy multinomial route (one rvs + logpmf per distinct N, as stats.py:132-148 does for long steps) on this box, for
                a few simulations, scaled to --sims.
One warm-up, then --repeats timed runs: minimum and median."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from cellranger_amd import engine as E  # noqa: E402
import emptydrops_numpy as R  # noqa: E402


def problem(n_features, n_candidates, seed=11):
    rs = np.random.RandomState(seed)
    p = np.exp(rs.normal(0, 2, n_features))
    umis = np.exp(rs.uniform(np.log(500), np.log(20000), n_candidates)).astype(np.uint32)
    return p / p.sum(), umis


def pilot_observed(c, p, umis):
    sim_n, tab, _, _ = c.emptydrops_simulate(p, umis, 32, seed=99)
    return np.median(tab, axis=1)[np.searchsorted(sim_n, umis)]


def time_sim(c, p, umis, obs, sims, repeats):
    ms = [c.emptydrops_simulate(p, umis, sims, seed=0, obs_loglk=obs, keep_table=False)[3] for _ in range(1 + repeats)][1:]
    return sorted(ms)


def sim_line(tag, c, p, umis, sims, repeats):
    obs = pilot_observed(c, p, umis)
    ms = time_sim(c, p, umis, obs, sims, repeats)
    draws = float(sims) * float(umis.max())
    print("simulation %-12s features=%d candidates=%d distinct_n=%d largest_n=%d sims=%d | kernel ms min=%.1f median=%.1f | %.2f G draws/s"
          % (tag, len(p), len(umis), len(np.unique(umis)), umis.max(), sims, ms[0], ms[len(ms) // 2], draws / ms[0] / 1e6), flush=True)
    return ms[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--features", type=int, default=36601)
    ap.add_argument("--candidates", type=int, default=100000)
    ap.add_argument("--sims", type=int, default=10000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    p, umis = problem(a.features, a.candidates)
    os.environ.pop("CRGPU_ED_LDS_FEATURES", None)
    c = E.Context(0)
    sim_line("production", c, p, umis, a.sims, a.repeats)
    sim_line("one_n", c, p, np.full(a.candidates, umis.max(), np.uint32), a.sims, a.repeats)
    p64, _ = problem(64, 1)
    sim_line("few_features", c, p64, umis, a.sims, a.repeats)
    c.close()
    os.environ["CRGPU_ED_LDS_FEATURES"] = "0"      # read when the context is created
    cg = E.Context(0)
    sim_line("global", cg, p, umis, a.sims, a.repeats)
    cg.close()
    os.environ.pop("CRGPU_ED_LDS_FEATURES")

    # the whole step on a planted well
    c = E.Context(0)
    indptr, indices, data, nf, kind = R.make_well(7, n_features=2000, n_cells=1000, n_ambient=40000, n_big_ambient=3000, n_small_cells=1000)
    V = len(kind)
    c.set_whitelist(0, np.arange(1 << 16, dtype=np.uint32), length=16)
    seen = np.zeros(c.n_canon, np.uint32)
    seen[:V] = 1
    c.set_counts(0, 0, seen)
    bc = np.repeat(np.arange(V, dtype=np.uint32), np.diff(indptr))
    m = c.assemble_matrix_dev(c.upload(bc), c.upload(indices.astype(np.uint32)), c.upload(data.astype(np.uint32)), len(indices))
    cells = np.flatnonzero(kind == 0).astype(np.uint64)
    call = E.CellCall(c, c.upload(cells), len(cells), {}, m)
    wall, kern, last = [], [], None
    for rep in range(1 + a.repeats):
        t0 = time.perf_counter()
        last = c.call_additional_cells(m, call, 10000, 30000, emptydrops_minimum_umis=100, num_sims=a.sims)
        if rep:
            wall.append((time.perf_counter() - t0) * 1e3)
            kern.append(last.metrics["sim_ms"])
    wall.sort()
    k3 = kind[last.eval_cols.astype(np.int64)]
    print("whole_step columns=%d nnz=%d features=%d candidates=%d distinct_n=%d sims=%d status=%d | call ms min=%.1f median=%.1f | simulation "
          "kernel ms min=%.1f (%.0f %% of the call) | small cells called %d of %d, large ambient droplets called %d of %d"
          % (V, len(indices), nf, len(last.eval_cols), last.metrics["n_distinct_n"], a.sims, last.status, wall[0], wall[len(wall) // 2],
             min(kern), 100 * min(kern) / wall[0], last.is_nonambient[k3 == 3].sum(), (k3 == 3).sum(), last.is_nonambient[k3 == 2].sum(),
             (k3 == 2).sum()), flush=True)
    if not a.no_cpu:
        from scipy import stats as sp_stats

        few = 4
        t0 = time.perf_counter()
        R.simulate_philox(last.profile_p, last.umis, few, seed=0)
        t_np = (time.perf_counter() - t0) / few
        dn = np.unique(last.umis)
        t0 = time.perf_counter()
        for _ in range(few):
            counts = np.zeros(len(last.profile_p), np.int64)
            prev = 0
            for n in dn:
                counts += np.ravel(sp_stats.multinomial.rvs(int(n - prev), last.profile_p, size=1))
                sp_stats.multinomial.logpmf(counts, int(n), p=last.profile_p)
                prev = n
        t_sp = (time.perf_counter() - t0) / few
        print("cpu whole_step simulation: numpy restatement %.3f s per simulation (%.0f s for %d; x%.0f of the kernel), scipy multinomial "
              "rvs + logpmf per distinct N %.3f s per simulation (%.0f s; x%.0f)"
              % (t_np, t_np * a.sims, a.sims, t_np * a.sims * 1e3 / min(kern), t_sp, t_sp * a.sims, t_sp * a.sims * 1e3 / min(kern)), flush=True)
    c.close()


if __name__ == "__main__":
    main()
