"""Time of Counts.probe_triplets_dev (BcUmiInfo::probe_counts on the device) on the cfg3 model.
usage (GPU box): python3 scripts/bench_probe_counts.py [--reads N] [--disorder F] [--probes P] [--repeats R] [--routes default,global]
The well keeps cfg3's shape at every size: 10 000 cells and 200 000 ambient barcodes per 10^9 reads, so a cell has as many
molecules as in the 1 B-read configuration.
Probes follow the features (probe sets are laid out gene by gene), except in a share F of the barcodes, whose probes are a
hash of the feature: those segments are out of order and must be sorted.  Every timed call runs on fresh counts (the result
is cached in the counts object otherwise); the clock is the host's around a call that ends in a device synchronise.
`global` forces every segment through the device radix sort (CRGPU_PROBE_SEG_CAP=0, read when the context is created).
Prints one line per route; under `rocprofv3 --kernel-trace --stats` the kernels of the feature-triplet family of the same run
(k_mt_count, k_mt_write, k_trip_counts) are the yardstick for k_pc_* and the k_cp_* compactions."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from cellranger_amd import engine as E  # noqa: E402
from cellranger_amd import synth as S  # noqa: E402


def run(route, n, disorder, n_probes, repeats):
    if route == "global":
        os.environ["CRGPU_PROBE_SEG_CAP"] = "0"
    else:
        os.environ.pop("CRGPU_PROBE_SEG_CAP", None)
    w = S.Workload(n_total=n, seed=S.SEED0 + 3, n_cells=max(1, n // 100_000), n_ambient=max(1, n // 5_000))
    c = E.Context(0)
    c.set_whitelist(0, w.wl_packed, length=16)
    c.set_key_layout(w.n_genes, w.umi_len, 1, 0)
    d = dict(cb=c.empty(n, np.uint32), cbq=c.empty((n, 16), np.uint8), fl=c.empty(n, np.uint8), umi=c.empty(n, np.uint32),
             uq=c.empty((n, 12), np.uint8), ft=c.empty(n, np.uint32), idx=c.empty(n, np.uint32))
    c.synth(w, 0, n, cb=d["cb"].ptr, cb_qualn=d["cbq"].ptr, umi=d["umi"].ptr, umi_qualn=d["uq"].ptr, feature=d["ft"].ptr,
            flags=d["fl"].ptr)
    c.match_and_count(d["cb"], d["fl"], n, d["idx"])
    c.correct(d["cb"], d["cbq"], d["fl"], n, d["idx"])
    ft, idx = d["ft"].to_host(), d["idx"].to_host()
    probe = (ft.astype(np.int64) * n_probes // w.n_genes)                       # ascending with the feature
    shuffled = ((idx.astype(np.uint64) * np.uint64(2654435761)) >> np.uint64(12)) % np.uint64(1000) < np.uint64(round(disorder * 1000))
    probe[shuffled] = ((ft[shuffled].astype(np.uint64) * np.uint64(2654435761)) >> np.uint64(7)) % np.uint64(n_probes)
    probe[ft == 0xFFFFFFFF] = -1
    d_pr = c.upload(probe.astype(np.int32))
    del ft, idx, probe, shuffled
    recs = c.records(n, w.umi_len, d["idx"], d["umi"], d["uq"], d["ft"], d["fl"], d_probe_idx=d_pr)
    times, nt, nm = [], 0, 0
    for rep in range(2 + repeats):   # the device pool settles in two rounds
        counts = c.count_records(recs)
        c.synchronize()
        t0 = time.perf_counter()
        nt = counts.probe_triplets_dev(n_probes)[3]
        c.synchronize()
        if rep >= 2:
            times.append(time.perf_counter() - t0)
        nm = counts.n_molecules
        counts.free()
    seg = [c.stat(k) for k in (12, 13, 14)]
    times.sort()
    print("probe_triplets_dev route=%s reads=%d molecules=%d triplets=%d disorder=%.2f n_probes=%d segments(wave,workgroup,global)=%s "
          "ms min=%.3f median=%.3f max=%.3f (%d calls)" % (route, n, nm, nt, disorder, n_probes, seg, times[0] * 1e3,
                                                         times[len(times) // 2] * 1e3, times[-1] * 1e3, len(times)), flush=True)
    c.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=100_000_000)
    ap.add_argument("--disorder", type=float, default=0.25)
    ap.add_argument("--probes", type=int, default=54_000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--routes", default="default,global")
    a = ap.parse_args()
    for route in a.routes.split(","):
        run(route, a.reads, a.disorder, a.probes, a.repeats)


main()
