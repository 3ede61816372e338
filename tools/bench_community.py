#!/usr/bin/env python3
"""Times the clustering of a reference graph (nabo_community_*: seeded synchronous Louvain, aggregation, component
split) on the GPU.  No pass / fail threshold: the step is new in this project, so there is no earlier figure to beat,
and leidenalg / igraph are not installed here, so there is no reference figure either.

    python tools/bench_community.py [--quick] [--nodes 1000000] [--comps 20] [--k 15] [--resolution 1.0]

The graph: Nabo's SNN graph of nabo_amd._synth.pca_like cells (`--comps` components) -- every cell lists its k nearest
cells, itself included, an edge weighs round(s / (2 (k - 1) - s), 2), s the neighbours both ends share
(nabo/_mapping.py:185-198); the k-NN and the counts come from the GPU.  --quick: 100 000 nodes.  Per case one JSON line,
appended to profiles/community_bench.jsonl: device ms of the sweeps, the aggregations, the finish (split, numbering, the
final modularity) and the whole run; sweeps and moves per level; the clusters, their modularity; the mean ms per sweep
over all levels; the wall time of the one call louvain_csr, the host-side graph preparation included.
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


def snn_graph(n, comps, k):
    import nabo_amd
    from nabo_amd._synth import pca_like
    X = pca_like(n, comps, seed=77)
    idx, _ = nabo_amd.knn(X, X, k)
    s = nabo_amd.snn_counts(idx, idx, k).astype(np.float64)
    w = np.round(s / (2.0 * (k - 1) - s), 2)
    keep = (s > 0).ravel()
    ptr = np.concatenate([[0], np.cumsum((s > 0).sum(axis=1))]).astype(np.int64)
    return ptr, idx.ravel()[keep], w.ravel()[keep]


def bench(n, comps, k, resolution, seed=4466):
    import nabo_amd
    from nabo_amd import _community, _lib
    ptr, nbr, w = snn_graph(n, comps, k)
    t0 = time.perf_counter()
    with _community.Community(ptr, nbr, w, resolution=resolution, seed=seed) as H:
        wall_create = time.perf_counter() - t0
        _, n_arcs, two_m = H.level_size()
        longest = int(np.diff(H.get_level()["ptr"]).max())
        H.run()                                    # warm-up: first launches
        t0 = time.perf_counter()
        labels, info = H.run()
        wall_run = time.perf_counter() - t0
    t0 = time.perf_counter()
    again, _ = nabo_amd.louvain_csr(ptr, nbr, w, resolution=resolution, seed=seed)
    wall_call = time.perf_counter() - t0
    hist, ms = info["history"], info["ms"]
    sweeps = sum(h[2] for h in hist)
    return {"bench": "community", "nodes": n, "comps": comps, "k": k, "resolution": resolution, "seed": seed, "arcs": n_arcs,
            "two_m": two_m, "longest_row": longest, "geometry": _community.geometry(), "device_ms": ms,
            "levels": [{"n": h[0], "n_next": h[1], "sweeps": h[2], "moved": h[3], "q": h[4]} for h in hist],
            "sweeps": sweeps, "sweep_ms_mean": ms["sweeps"] / max(sweeps, 1), "n_clusters": info["n_clusters"], "q": info["q"],
            "same_labels_again": bool(np.array_equal(labels, again)), "create_wall_seconds": wall_create,
            "run_wall_seconds": wall_run, "louvain_csr_wall_seconds": wall_call, "lib": _lib.so_digest()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--nodes", type=int, nargs="*", default=None)
    ap.add_argument("--comps", type=int, default=20)
    ap.add_argument("--k", type=int, default=15)
    ap.add_argument("--resolution", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "community_bench.jsonl"))
    a = ap.parse_args()
    for n in a.nodes or ([100000] if a.quick else [1000000]):
        r = bench(n, a.comps, a.k, a.resolution)
        line = json.dumps(r)
        print(line, flush=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
