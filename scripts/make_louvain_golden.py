#!/usr/bin/env python
"""Record tests/golden/louvain_reference.npz from networkx 3.4.2's serial Louvain (CPU only).

Per kNN fixture <name> of tests/louvain_numpy.py's golden_fixtures(): <name>_indptr, <name>_indices = the neighbour matrix (row-wise
ascending, the form run_graph_clustering hands on), <name>_q0 and <name>_qfinal f64[16] = the modularity of the first and of the last
partition networkx.community.louvain_partitions yields on the union graph for the seeds 0 .. 15, <name>_spread f64[2] = maximum minus
minimum of each.  names = the fixtures.

Expected integers of the round form are NOT stored: the tests compute them from the restatement.  The file exists because networkx
and scikit-learn need not be present where the GPU tests run.  The restatement's own figures are printed beside networkx's.

    python scripts/make_louvain_golden.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import louvain_numpy as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "louvain_reference.npz")
SEEDS = range(16)


def main():
    import networkx as nx

    assert nx.__version__ == "3.4.2", "the reference is networkx 3.4.2, this is %s" % nx.__version__
    out, names = {}, []
    for name, (indptr, indices) in R.golden_fixtures().items():
        graph = R.union(indptr, indices)
        rows = R.csr_rows(graph[0])
        assert not (rows == graph[1]).any(), "%s has a self-loop: networkx counts it twice" % name
        G = nx.Graph()
        G.add_nodes_from(range(len(indptr) - 1))
        G.add_edges_from(zip(rows.tolist(), graph[1].tolist()))
        q0, qf = [], []
        for seed in SEEDS:
            parts = list(nx.community.louvain_partitions(G, seed=seed))
            q0.append(nx.community.modularity(G, parts[0])), qf.append(nx.community.modularity(G, parts[-1]))
        q0, qf = np.array(q0), np.array(qf)
        mine = R.louvain(indptr, indices)
        M = float(mine["M"])
        print("%-18s n %5d nnz %7d: networkx level 0 %.5f .. %.5f, final %.5f .. %.5f; the round form level 0 %.5f, final %.5f, rounds %s, "
              "communities %s" % (name, len(indptr) - 1, len(graph[1]), q0.min(), q0.max(), qf.min(), qf.max(), mine["S"][0] / M ** 2,
                                  mine["S"][-1] / M ** 2, mine["rounds"], mine["communities"]))
        names.append(name)
        out.update({name + "_indptr": np.asarray(indptr, np.int64), name + "_indices": np.asarray(indices, np.int32), name + "_q0": q0,
                    name + "_qfinal": qf, name + "_spread": np.array([q0.max() - q0.min(), qf.max() - qf.min()])})
    out["names"] = np.array(names)
    np.savez_compressed(OUT, **out)
    print("wrote %s: %d bytes" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
