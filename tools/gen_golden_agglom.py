"""Writes tests/golden/agglom.npz: what the agglomeration tests' numpy yardstick (tests/_agglom_ref.py) does on the graph
of tests/golden/community.npz -- rounds, passes, the merge list, the peak, the modularity at the cuts 5, 8, 10, 20 and 40
-- and, beside it, the modularity of networkx's greedy_modularity_communities (Clauset-Newman-Moore, one merge at a time)
at the same cuts, scored by the exact formula of include/nabo_community.h.  A cut below the number of connected components
cannot be reached by either and is recorded as NaN.  No threshold is set against networkx: the file records the measured
differences.

    python tools/gen_golden_agglom.py

Needs networkx (3.4.2 when the file was written); the tests need only the file."""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
import _agglom_ref as ar  # noqa: E402
import _community_ref as cr  # noqa: E402

CUTS = (5, 8, 10, 20, 40)


def main():
    import networkx as nx
    d = np.load(os.path.join(REPO, "tests", "golden", "community.npz"))
    ptr, nbr, w = d["ptr"], d["nbr"].astype(np.int64), d["w"]
    res = ar.run(ptr, nbr, w)
    lv0, two_m = res["lv0"], res["two_m"]
    n = lv0.n
    G = nx.Graph()
    G.add_nodes_from(range(n))
    for i, j, a in zip(lv0.src.tolist(), lv0.dst.tolist(), lv0.a.tolist()):                  # the quantised simple graph
        G.add_edge(i, j, weight=a)
    for i, s in enumerate(lv0.inn.tolist()):
        if s:
            G.add_edge(i, i, weight=s)
    components = nx.number_connected_components(G)
    assert components == res["n_end"]
    q_cut, nx_q = np.full(len(CUTS), np.nan), np.full(len(CUTS), np.nan)
    for at, c in enumerate(CUTS):
        if c < components:
            print("%d clusters: below the graph's %d components" % (c, components))
            continue
        labels, C, q_cut[at] = ar.cut(res, c)
        assert C == c and q_cut[at] == cr.label_q(lv0, two_m, labels, 1.0)
        lab = np.zeros(n, dtype=np.int64)
        parts = nx.community.greedy_modularity_communities(G, weight="weight", cutoff=c, best_n=c)
        assert len(parts) == c
        for x, members in enumerate(parts):
            lab[list(members)] = x
        nx_q[at] = cr.label_q(lv0, two_m, lab, 1.0)
        print("%d clusters: yardstick Q = %.6f, networkx CNM %.6f, apart by %+.6f" % (c, q_cut[at], nx_q[at], q_cut[at] - nx_q[at]))
    lab = np.zeros(n, dtype=np.int64)
    parts = nx.community.greedy_modularity_communities(G, weight="weight")
    for x, members in enumerate(parts):
        lab[list(members)] = x
    nx_peak_q = cr.label_q(lv0, two_m, lab, 1.0)
    peak_q = float(res["q_path"][res["peak"]])
    print("%d rounds, %d passes, %d merges; the peak: %d clusters at Q = %.16f; networkx CNM's: %d clusters at Q = %.16f"
          % (res["rounds"], res["passes"], len(res["merges"]), n - res["peak"], peak_q, len(parts), nx_peak_q))
    out = os.path.join(REPO, "tests", "golden", "agglom.npz")
    np.savez_compressed(out, rounds=np.int64(res["rounds"]), passes=np.int64(res["passes"]), merges=res["merges"],
                        peak=np.int64(res["peak"]), peak_q=np.float64(peak_q), n_end=np.int64(res["n_end"]), cuts=np.array(CUTS),
                        q_cut=q_cut, nx_q=nx_q, nx_peak_q=np.float64(nx_peak_q), nx_peak_clusters=np.int64(len(parts)),
                        networkx_version=np.array(nx.__version__))
    print("wrote %s (%d bytes)" % (out, os.path.getsize(out)))


if __name__ == "__main__":
    main()
