"""Where a tile of k_correct_umis_tiled and a boundary of k_correct_umis_edges spend their time: phase attribution from a
-DUC_PHASE_TIMING build.
usage (GPU box): CRGPU_LIB_PATH=cellranger_amd/variants/libcrgpu_ucphases.so python3 scripts/umi_phases.py [n_reads]
Thread 0 of every workgroup adds the shader-clock ticks between the phase marks to sixteen device counters; printed as the
share of each phase over all tiles (all boundaries) of one count call on the cfg3 workload."""
import ctypes
import sys

import numpy as np

sys.path.insert(0, ".")
from cellranger_amd import _lib  # noqa: E402
from cellranger_amd import engine as E  # noqa: E402
from cellranger_amd import synth as S  # noqa: E402

TILE = [(0, "staging loads arrived"), (1, "heads + LDS stores"), (2, "head scan"), (3, "bounds + inserts"), (4, "search"),
        (5, "hash clear")]
EDGE = [(14, "walk over the boundaries in between"), (9, "hash clear + staging"), (10, "inserts"), (11, "search")]


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000_000
    w = S.Workload(n_total=n, seed=S.SEED0 + 3)
    c = E.Context(0)
    c.set_whitelist(0, w.wl_packed, length=16)
    c.set_key_layout(w.n_genes, w.umi_len, 1, 0)
    d = dict(cb=c.empty(n, np.uint32), cbq=c.empty((n, 16), np.uint8), fl=c.empty(n, np.uint8), umi=c.empty(n, np.uint32),
             uq=c.empty((n, 12), np.uint8), ft=c.empty(n, np.uint32), idx=c.empty(n, np.uint32))
    c.synth(w, 0, n, cb=d["cb"].ptr, cb_qualn=d["cbq"].ptr, umi=d["umi"].ptr, umi_qualn=d["uq"].ptr, feature=d["ft"].ptr,
            flags=d["fl"].ptr)
    c.match_and_count(d["cb"], d["fl"], n, d["idx"])
    c.correct(d["cb"], d["cbq"], d["fl"], n, d["idx"])
    recs = c.records(n, w.umi_len, d["idx"], d["umi"], d["uq"], d["ft"], d["fl"])
    keys = c.empty(n, np.uint64)
    lib = _lib.load()
    out = (ctypes.c_ulonglong * 16)()
    for rep in range(2):   # the second call is the one reported: the read clears the counters
        nk = c.build_keys(recs, keys)
        c.count_keys(keys, nk).free()
        c.synchronize()
        assert lib.crgpu_debug_uc_phases(out) == 0
    v = np.array(list(out), dtype=np.float64)
    print("n_keys %d: %d tiles, %d edge segments" % (nk, int(v[6]), int(v[12])))
    for title, rows, per, cnt in (("k_correct_umis_tiled", TILE, "tile", v[6]), ("k_correct_umis_edges", EDGE, "segment", v[12])):
        tot = sum(v[i] for i, _ in rows)
        print("%s: %.0f ticks per %s" % (title, tot / max(cnt, 1.0), per))
        for i, name in rows:
            print("  %-40s %6.2f %%" % (name, 100.0 * v[i] / max(tot, 1.0)))


main()
