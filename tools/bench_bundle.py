#!/usr/bin/env python3
"""Times edge bundling (nabo_bundle_run: density-guided advection, include/nabo_bundle.h) on the GPU.  No pass / fail
threshold: the step has no earlier version in this project and no reference figure (datashader is not installed; its
hammer_bundle runs Python and numba on one core).

    python tools/bench_bundle.py [--quick] [--nodes 100000 [1000000 ...]] [--k 15] [--accuracy 500] [--append]

The graph: `--nodes` positions drawn from 40 seeded Gaussian blobs in the plane, standing in for a layout, each node joined
to its k Euclidean nearest neighbours there (nabo_amd.knn), a pair kept once if the two lists share a neighbour
(nabo_amd.snn_counts): an SNN graph on a layout, most of whose edges are shorter than one target segment.  Default sizes:
100 000 and 1 000 000 nodes; --quick: 20 000.  Prints one JSON line per size: device ms per phase of the run (HIP events,
nabo_bundle_last_ms), the wall time of the call, the points the edges end with, and point-steps per second of the advect
phase (every point of every edge in every advection step, counted from the points each round ends with).  --append adds
the lines to profiles/bundle_bench.jsonl.
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


def blob_graph(n, k, seed=11):
    import nabo_amd
    rng = np.random.default_rng(seed)
    centres = rng.random((40, 2)) * 100
    pos = centres[rng.integers(0, 40, size=n)] + rng.normal(size=(n, 2)) * 3.0
    idx, _ = nabo_amd.knn(pos, pos, k, metric=nabo_amd.EUCLIDEAN, drop_first=True)
    s = nabo_amd.snn_counts(idx, idx, k)
    src = np.repeat(np.arange(n, dtype=np.int64), k)
    dst = idx.reshape(-1).astype(np.int64)
    keep = (s.reshape(-1) > 0) & (src != dst)
    src, dst = src[keep], dst[keep]
    key = np.minimum(src, dst) * n + np.maximum(src, dst)
    _, first = np.unique(key, return_index=True)
    first.sort()
    return pos, src[first], dst[first]


def bench(n, k, accuracy):
    from nabo_amd import _bundle, _lib
    pos, src, dst = blob_graph(n, k)
    with _bundle.Bundle(pos, src, dst, accuracy=accuracy) as B:
        B.resample()                                   # warm-up: first launches, the buffers' first allocation
        t0 = time.perf_counter()
        B.run()
        wall = time.perf_counter() - t0
        ms = B.last_ms()
        off, _ = B.get_points()
    p = B.params
    rounds, d = 0, p["decay"]
    for _ in range(p["iterations"]):
        if (p["initial_bandwidth"] * d) * accuracy < 2:
            break
        rounds, d = rounds + 1, d * p["decay"]
    steps = float(off[-1]) * rounds * p["advect_iterations"]
    return {"bench": "bundle", "nodes": n, "k": k, "edges": int(len(src)), "accuracy": accuracy, "rounds": rounds,
            "points": int(off[-1]), "longest_edge_points": int(np.diff(off).max()),
            "edges_of_two_points": int((np.diff(off) == 2).sum()), "geometry": _bundle.geometry(),
            "device_ms": ms, "wall_seconds": wall, "advect_point_steps": steps,
            "advect_point_steps_per_second": steps / (ms["advect"] * 1e-3) if ms["advect"] > 0 else None,
            "so": _lib.so_digest()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--nodes", type=int, nargs="*", default=None)
    ap.add_argument("--k", type=int, default=15)
    ap.add_argument("--accuracy", type=int, default=500)
    ap.add_argument("--append", action="store_true")
    a = ap.parse_args()
    sizes = a.nodes or ([20000] if a.quick else [100000, 1000000])
    for n in sizes:
        line = json.dumps(bench(n, a.k, a.accuracy))
        print(line, flush=True)
        if a.append:
            os.makedirs(os.path.join(REPO, "profiles"), exist_ok=True)
            with open(os.path.join(REPO, "profiles", "bundle_bench.jsonl"), "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    sys.exit(main())
