#!/usr/bin/env python3
"""Times the ForceAtlas2 layout (nabo_layout_run: every pair summed) on the GPU.  No pass / fail threshold: the step has
no earlier version in this project; the only reference figure is its notebook's 5 s for 1 414 nodes x 500 iterations
with Barnes-Hut (2_mapping.ipynb).

    python tools/bench_layout.py [--quick] [--nodes 100000] [--k 15] [--iters 50]

The graph: `--nodes` cells of nabo_amd._synth.pca_like (30 components), each joined to its k Euclidean nearest
neighbours (nabo_amd.knn) with the SNN weight s / (2 (k - 1) - s) of the s neighbours the two lists share
(nabo_amd.snn_counts), pairs without a shared neighbour dropped; --quick: 20 000 nodes.  Prints one JSON line: ms per
kernel per iteration (means over the run's last 16 iterations, HIP events), ms of the whole run per iteration, pair terms
per second of the repulsion kernel, and that rate as a fraction of the loop's issue bound: 64 pair terms
per ISSUE_CYCLES cycles of one SIMD, counted from the loop as built with the per-instruction issue costs of one wave's
stream, times 4 SIMDs x 256 CUs x 2.4 GHz.
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

# the repulsion loop as built: per pair term v_rcp_f32 (8 cycles) and 8 plain float32 operations (4
# each; where the compiler packs two of them into one v_pk_*_f32, that instruction counts as the two it replaces)
PAIRS_PER_ISSUE = 64
ISSUE_CYCLES = 8 + 8 * 4
SIMDS, CLOCK_HZ = 4 * 256, 2.4e9


def snn_graph(n, k, seed=11):
    import nabo_amd
    from nabo_amd._synth import pca_like
    X = pca_like(n, 30, seed)
    idx, _ = nabo_amd.knn(X, X, k, metric=nabo_amd.EUCLIDEAN, drop_first=True)
    s = nabo_amd.snn_counts(idx, idx, k).astype(np.float64)
    keep = s > 0
    w = np.where(keep, s / np.maximum(2.0 * (k - 1) - s, 1.0), 0.0)
    ptr = np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.int64)
    return ptr, idx[keep].astype(np.int64), w[keep]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--nodes", type=int, default=None)
    ap.add_argument("--k", type=int, default=15)
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    n = a.nodes or (20000 if a.quick else 100000)
    from nabo_amd import _layout, _lib
    ptr, nbr, w = snn_graph(n, a.k)
    pos0 = np.random.default_rng(0).random((n, 2))
    with _layout.Layout(ptr, nbr, w) as L:
        L.set_state(pos0[:, 0], pos0[:, 1])
        L.run(2)                                      # warm-up: first launches, the edge factors' upload
        L.set_state(pos0[:, 0], pos0[:, 1])
        t0 = time.perf_counter()
        done = L.run(a.iters)
        wall = time.perf_counter() - t0
        ms = L.last_ms()
        s = L.get_state()
    pairs = float(n) * float(n)
    rate = pairs / (ms["repulsion"] * 1e-3)
    bound = PAIRS_PER_ISSUE / ISSUE_CYCLES * SIMDS * CLOCK_HZ
    print(json.dumps({"bench": "layout_fa2", "nodes": n, "k": a.k, "arcs": int(len(nbr)), "iterations": a.iters, "done": done,
                      "geometry": dict(zip(("i_block", "j_tile", "n_splits"), _layout.geometry(n))),
                      "ms_per_iteration": {k: ms[k] for k in _layout.KERNELS}, "timed_iterations": ms["n_timed"],
                      "run_ms_per_iteration": ms["run"] / max(done, 1), "wall_seconds": wall,
                      "pair_terms_per_iteration": pairs, "pair_terms_per_second": rate, "issue_bound_pair_terms_per_second": bound,
                      "fraction_of_issue_bound": rate / bound, "finite": bool(np.isfinite(s["x"]).all() and np.isfinite(s["y"]).all()),
                      "so": _lib.so_digest()}), flush=True)


if __name__ == "__main__":
    sys.exit(main())
