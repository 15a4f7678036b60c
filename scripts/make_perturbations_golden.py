#!/usr/bin/env python
"""Record the reference's own grouping of the cells for the hand cases of tests/perturbations_numpy.py
-> tests/golden/perturbations_reference.npz.

    python scripts/make_perturbations_golden.py <reference checkout>/lib/python

Runs on the CPU.  At record time it loads cellranger.feature.crispr.measure_perturbations from the reference with the cellranger and
tenkit modules it imports stubbed (they need HDF5 and numexpr; _get_target_info and _get_ps_clusters use pandas and numpy only), except
cellranger.constants, which holds FILTER_LIST and loads as it is.  Nothing of the reference is copied: the file holds, per case, what
_get_ps_clusters returned for the fixture of tests/perturbations_numpy.py: the cluster of every barcode, the names in cluster order, and
`sorted_join` = whether every multi-target name came out with its parts in sorted order.  The reference joins list(set(...)): the order
of a multi-target name depends on the hash seed of the recording process, so the test compares the partition of the cells always and
the numbering and the names only where sorted_join holds."""
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import perturbations_numpy as P  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "perturbations_reference.npz")


class _Anything:
    def __init__(self, *a, **k):
        pass

    def __call__(self, *a, **k):
        return _Anything()

    def __getattr__(self, name):
        return _Anything()


class _Stub(types.ModuleType):
    __path__ = []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return _Anything()


def load_reference(ref_path):
    sys.path.insert(0, ref_path)
    import cellranger.constants  # noqa: F401  (the real one: FILTER_LIST)

    for name in ("cellranger.analysis", "cellranger.analysis.analysis_types", "cellranger.analysis.diffexp", "cellranger.rna", "cellranger.rna.library",
                 "tenkit", "tenkit.stats"):
        sys.modules[name] = _Stub(name)
        parent, _, leaf = name.rpartition(".")
        if parent in sys.modules:
            setattr(sys.modules[parent], leaf, sys.modules[name])
    for _ in range(20):
        try:
            import cellranger.feature.crispr.measure_perturbations as mp

            return mp
        except ImportError as e:      # a third-party module that is not installed: stub it and try again
            if not e.name or e.name in sys.modules:
                raise
            sys.modules[e.name] = _Stub(e.name)
    raise RuntimeError("the reference module does not load")


def main(ref_path):
    import pandas as pd

    mp = load_reference(ref_path)
    out = {}
    for case in sorted(P.HAND_CASES):
        feature_ref, by_feature, ignore_multiples, _, _ = P.HAND_CASES[case]
        ref_table = pd.DataFrame(feature_ref)
        calls = pd.DataFrame({"num_features": [v[1] for v in P.CALLS.values()], "feature_call": [v[0] for v in P.CALLS.values()]}, index=list(P.CALLS))
        info = mp._get_target_info(ref_table)
        per_bc, names = mp._get_ps_clusters(info, calls, [b.encode() for b in P.BARCODES], by_feature, ignore_multiples)
        ordered = [names[c] for c in sorted(names)]
        out[case + ".clusters"] = np.asarray(per_bc, np.int64)
        out[case + ".names"] = np.array(ordered)
        out[case + ".sorted_join"] = np.array(all(n.split("|") == sorted(n.split("|")) for n in ordered) or by_feature)
        print(case, list(per_bc), ordered, bool(out[case + ".sorted_join"]))
    np.savez(OUT, **out)
    print("wrote", OUT)


if __name__ == "__main__":
    main(sys.argv[1])
