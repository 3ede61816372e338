#!/usr/bin/env python3
"""Times the differentiation potential of a reference graph (nabo_potential_*: K x = b by Jacobi-preconditioned
conjugate gradients) on the GPU.  No pass / fail threshold: the step is new in this project.

    python tools/bench_potential.py [--quick] [--nodes 100000 1000000] [--comps 20] [--k 15] [--tol 1e-10]
    python tools/bench_potential.py --reference [--nodes 1000 3000]

The graph: Nabo's SNN graph of nabo_amd._synth.pca_like cells (`--comps` components) -- every cell lists its k nearest
cells, itself included, edges with at least one shared neighbour are kept (nabo/_mapping.py:185-198; the weights play no
part here); the k-NN and the counts come from the GPU.  --quick: 100 000 nodes only.  Per case one JSON line, appended to
profiles/potential_bench.jsonl: the iterations to `tol`, device ms of prepare, the iterations and finish, ms per
iteration, and the effective bytes per second of the product, counting per iteration arcs * 4 B of neighbour ids, 8 B
gathered per arc, and the vectors the product streams (row pointers 8 B, c, p_i and q: 32 B per node); the other two
kernels of an iteration stream another 88 B per node (update: p, q, x, res, 1/c read, x, res written; direction: res, 1/c, p read, p written), reported apart.
--reference: the dense route of the reference (numpy.linalg.pinv of I - A/D) on small graphs, on this host's CPU; needs
no GPU.
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
    s = nabo_amd.snn_counts(idx, idx, k)
    keep = (s > 0).ravel()
    ptr = np.concatenate([[0], np.cumsum((s > 0).sum(axis=1))]).astype(np.int64)
    return ptr, idx.ravel()[keep].astype(np.int64)


def bench(n, comps, k, tol, max_iter):
    import nabo_amd
    from nabo_amd import _lib, _potential
    ptr, nbr = snn_graph(n, comps, k)
    r = np.random.default_rng(5).normal(size=n)
    t0 = time.perf_counter()
    with _potential.Potential(ptr, nbr, tol=tol, max_iter=max_iter) as H:
        wall_create = time.perf_counter() - t0
        _, n_arcs, n_long = H.graph_size()
        H.solve(r)                                   # warm-up: first launches
        t0 = time.perf_counter()
        V, info = H.solve(r)
        wall_run = time.perf_counter() - t0
    t0 = time.perf_counter()
    again, _ = nabo_amd.diff_potential_csr(ptr, nbr, r, tol=tol, max_iter=max_iter)
    wall_call = time.perf_counter() - t0
    ms, it = info["ms"], max(info["iterations"], 1)
    per_it = ms["iterate"] / it
    product_bytes = n_arcs * 12 + n * 32
    return {"bench": "potential", "nodes": n, "comps": comps, "k": k, "tol": tol, "arcs": n_arcs, "long_rows": n_long,
            "geometry": _potential.geometry(), "iterations": info["iterations"], "status": info["status"],
            "residual": info["residual"], "true_residual": info["true_residual"], "n_components": info["n_components"],
            "device_ms": ms, "iteration_ms": per_it, "product_bytes_per_iteration": product_bytes,
            "vector_bytes_per_iteration": n * 88,
            "effective_bytes_per_second_whole_iteration": (product_bytes + n * 88) / (per_it * 1e-3) if per_it > 0 else None,
            "same_bits_again": bool(V.tobytes() == again.tobytes()), "create_wall_seconds": wall_create,
            "run_wall_seconds": wall_run, "diff_potential_csr_wall_seconds": wall_call, "lib": _lib.so_digest()}


def reference(n, centres=8):
    """the dense route on an n-node Gaussian-blob SNN graph, on this host's CPU"""
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import _community_ref as cr
    import _potential_ref as pr
    ptr, nbr, _ = cr.blob_snn_graph(n=n, centres=centres)
    G = pr.Graph(ptr, nbr)
    t0 = time.perf_counter()
    V = pr.pinv_potential(G)
    dense = time.perf_counter() - t0
    t0 = time.perf_counter()
    W, info = pr.potential(ptr, nbr)
    sparse = time.perf_counter() - t0
    return {"bench": "potential_reference", "nodes": n, "arcs": int(len(G.src)), "dense_pinv_cpu_seconds": dense,
            "numpy_pcg_cpu_seconds": sparse, "iterations": info["iterations"], "max_abs_difference": float(np.abs(V - W).max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--reference", action="store_true")
    ap.add_argument("--nodes", type=int, nargs="*", default=None)
    ap.add_argument("--comps", type=int, default=20)
    ap.add_argument("--k", type=int, default=15)
    ap.add_argument("--tol", type=float, default=1e-10)
    ap.add_argument("--max-iter", type=int, default=10000)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "potential_bench.jsonl"))
    a = ap.parse_args()
    if a.reference:
        cases = [reference(n) for n in a.nodes or [1000, 3000]]
    else:
        cases = (bench(n, a.comps, a.k, a.tol, a.max_iter) for n in a.nodes or ([100000] if a.quick else [100000, 1000000]))
    for r in cases:
        line = json.dumps(r)
        print(line, flush=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
