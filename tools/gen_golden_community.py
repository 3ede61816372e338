"""Writes tests/golden/community.npz: the 3 000-node Gaussian-blob SNN graph the community tests run on, the modularity
networkx's louvain_communities reaches on it (seeds 0-4 at resolutions 0.5, 1, 2; Q by the exact formula of
include/nabo_community.h from networkx's partitions), what the tests' numpy yardstick (tests/_community_ref.py) reaches,
and the measured distance between the exact modularity and a restatement of Graph.calc_modularity's float loops.

    python tools/gen_golden_community.py

Needs networkx (3.4.2 when the file was written); the tests need only the file."""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
import _community_ref as cr  # noqa: E402

GAMMAS = (0.5, 1.0, 2.0)
SEEDS = (0, 1, 2, 3, 4)


def main():
    import networkx as nx
    ptr, nbr, w = cr.blob_snn_graph()
    lv0, two_m = cr.level0(ptr, nbr, w)
    n = lv0.n
    G = nx.Graph()
    G.add_nodes_from(range(n))
    for i in range(n):
        for e in range(int(ptr[i]), int(ptr[i + 1])):
            G.add_edge(i, int(nbr[e]), weight=float(w[e]))           # a pair listed again keeps its last weight
    nx_q = np.zeros((len(GAMMAS), len(SEEDS)))
    ref_q = np.zeros(len(GAMMAS))
    ref_nc = np.zeros(len(GAMMAS), dtype=np.int64)
    ref_labels = np.zeros((len(GAMMAS), n), dtype=np.int32)
    for a, gamma in enumerate(GAMMAS):
        for b, seed in enumerate(SEEDS):
            lab = np.zeros(n, dtype=np.int64)
            for c, members in enumerate(nx.community.louvain_communities(G, weight="weight", resolution=gamma, seed=seed)):
                lab[list(members)] = c
            nx_q[a, b] = cr.label_q(lv0, two_m, lab, gamma)
        labels, info = cr.louvain(ptr, nbr, w, resolution=gamma)
        ref_q[a], ref_nc[a], ref_labels[a] = info["q"], info["n_clusters"], labels
        mono = all(x[4] <= y[4] for x, y in zip(info["history"], info["history"][1:]))
        print("resolution %g: yardstick Q = %.5f in %d clusters (%s over levels); networkx %d: %.5f .. %.5f"
              % (gamma, ref_q[a], ref_nc[a], "monotone" if mono else "NOT monotone", len(SEEDS), nx_q[a].min(), nx_q[a].max()))
    at = GAMMAS.index(1.0)
    loops, adds, max_edges = cr.reference_loops_q(ptr, nbr, w, ref_labels[at])
    exact = cr.label_q(lv0, two_m, ref_labels[at], 1.0)
    print("calc_modularity's float loops: %.17g, exact %.17g, apart by %.3g after %d additions (bound %.3g)"
          % (loops, exact, abs(loops - exact), adds, cr.loops_bound(adds, max_edges)))
    out = os.path.join(REPO, "tests", "golden", "community.npz")
    np.savez_compressed(out, ptr=ptr, nbr=nbr.astype(np.int32), w=w, two_m=np.int64(two_m), gammas=np.array(GAMMAS),
                        seeds=np.array(SEEDS), nx_q=nx_q, ref_q=ref_q, ref_n_clusters=ref_nc, ref_labels=ref_labels,
                        loops_q=np.float64(loops), loops_diff=np.float64(abs(loops - exact)), loops_adds=np.int64(adds),
                        networkx_version=np.array(nx.__version__))
    print("wrote %s (%d bytes)" % (out, os.path.getsize(out)))


if __name__ == "__main__":
    main()
