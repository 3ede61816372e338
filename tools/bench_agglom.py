#!/usr/bin/env python3
"""Times the greedy modularity agglomeration of a reference graph (include/nabo_agglom.h: match passes, the ordering of a
round's pairs, the aggregations; then a cut) on the GPU.  No pass / fail threshold: the step is new in this project and
`hac` is not installed here, so there is no reference figure.  The yardstick beside it is this project's Louvain run
(nabo_community_run) on the same graph and the same handle: its device time, its clusters and its modularity.

    python tools/bench_agglom.py [--quick] [--nodes 100000 1000000] [--comps 20] [--k 15]

The graph is that of tools/bench_community.py: Nabo's SNN graph of nabo_amd._synth.pca_like cells, k nearest cells each,
the k-NN and the shared-neighbour counts from the GPU.  --quick: 100 000 nodes only.  Per case one JSON line, appended to
profiles/agglom_bench.jsonl: device ms of the passes, the ordering, the aggregations and the whole run; rounds, passes and
merges; the clusters and the modularity at the peak; the mean ms per pass; the wall time of the cuts at the peak and at
10 clusters (if the graph has that few components); the Louvain figures.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

from bench_community import snn_graph  # noqa: E402


def bench(n, comps, k):
    from nabo_amd import _community, _lib
    ptr, nbr, w = snn_graph(n, comps, k)
    with _community.Community(ptr, nbr, w) as H:
        _, n_arcs, two_m = H.level_size()
        longest = int(np.diff(H.get_level()["ptr"]).max())
        H.agglomerate()                            # warm-up: first launches, the buffers
        t0 = time.perf_counter()
        info = H.agglomerate()
        wall_run = time.perf_counter() - t0
        t0 = time.perf_counter()
        labels, n_peak, q_peak = H.cut(0)
        wall_cut = time.perf_counter() - t0
        cut10 = None
        if info["n_end"] <= 10 <= n:
            t0 = time.perf_counter()
            _, _, q10 = H.cut(10)
            cut10 = {"q": q10, "wall_seconds": time.perf_counter() - t0}
        same = bool(np.array_equal(H.agglomerate()["merges"], info["merges"]) and np.array_equal(H.cut(0)[0], labels))
        H.run()                                    # the yardstick: Louvain on the same graph, warmed up the same way
        _, louvain = H.run()
    ms = info["ms"]
    per_round = np.bincount(info["merges"][:, 2], minlength=info["rounds"]).tolist() if info["rounds"] else []
    return {"bench": "agglom", "nodes": n, "comps": comps, "k": k, "arcs": n_arcs, "two_m": two_m, "longest_row": longest,
            "geometry": _community.geometry()[:2], "device_ms": ms, "rounds": info["rounds"], "passes": info["passes"],
            "merges": int(len(info["merges"])), "merges_per_round": per_round, "n_end": info["n_end"],
            "pass_ms_mean": ms["passes"] / max(info["passes"], 1), "peak_clusters": n_peak, "peak_q": q_peak,
            "cut_peak_wall_seconds": wall_cut, "cut_10": cut10, "same_bytes_again": same, "run_wall_seconds": wall_run,
            "louvain": {"device_ms": louvain["ms"], "n_clusters": louvain["n_clusters"], "q": louvain["q"]}, "lib": _lib.so_digest()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--nodes", type=int, nargs="*", default=None)
    ap.add_argument("--comps", type=int, default=20)
    ap.add_argument("--k", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "agglom_bench.jsonl"))
    a = ap.parse_args()
    for n in a.nodes or ([100000] if a.quick else [100000, 1000000]):
        r = bench(n, a.comps, a.k)
        line = json.dumps(r)
        print(line, flush=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
