#!/usr/bin/env python3
"""Times the UMAP embedding (nabo_umap_*: exact k-NN, fuzzy graph, synchronous epochs) on the GPU.  No pass / fail
threshold: the step is new in this project, so there is no earlier figure to beat, and umap-learn is not installed here,
so there is no reference figure either.

    python tools/bench_umap.py [--quick] [--cells 100000 1000000] [--comps 50] [--k 15] [--epochs 200]

The cells: nabo_amd._synth.pca_like (`--comps` components); --quick: 20 000 cells.  Per case one JSON line, appended to
profiles/umap_bench.jsonl: device ms of the k-NN, of the graph build (parts B and C of include/nabo_umap.h) and of the
whole run of epochs; ms of the epoch kernel as the mean over the run's last 16 epochs; the arcs fired and the negative
samples drawn in the LAST epoch, and from them arcs fired per second and gathered bytes per second (one position of
8 dims bytes per fired arc and per sample, the node's own not counted); the wall time of the one call umap_fit.

The gather rate stands beside the 16.8-18.8 TB/s README records for rows gathered from a table that one XCD's L2 holds.
That figure is an UPPER MARK, not a target: at 1M cells the position table is 16 MB (24 MB in 3 dimensions), four to
six times one XCD's 4 MiB L2, the gathered rows are 16 or 24 bytes and not 1 152, and every fired term also pays one
or two float64 pow.  Which of the two bounds the kernel is not known; this tool only reports.
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

L2_RESIDENT_GATHER_TBS = (16.8, 18.8)


def bench(n, comps, k, epochs, dims, seed=0):
    import nabo_amd
    from nabo_amd import _lib, _umap
    from nabo_amd._synth import pca_like
    X = pca_like(n, comps, seed=77)
    a, b = nabo_amd.find_ab_params(1.0, 0.1)
    y0 = _umap.start_positions("pca", X, n, dims, seed)
    with _umap.Umap(n, dims, n_epochs=epochs, a=a, b=b, seed=seed) as U:
        U.fit_knn(X, k)
        U.set_embedding(y0)
        U.run(2)                                   # warm-up: first launches
        U.rewind()
        U.set_embedding(y0)
        t0 = time.perf_counter()
        done = U.run()
        wall_run = time.perf_counter() - t0
        ms, c = U.last_ms(), U.last_epoch_counts()
        _, _, ptr, _, _ = U.graph()
        ok = bool(np.isfinite(U.get_embedding()).all())
    fired, drawn = int(c["n_attr"].sum()), int(c["n_neg"].sum())
    gathered = (fired + drawn) * dims * 8
    t0 = time.perf_counter()
    nabo_amd.umap_fit(X, k, dims, n_epochs=epochs, seed=seed)
    wall_call = time.perf_counter() - t0
    deg = np.diff(ptr)
    return {"bench": "umap", "cells": n, "comps": comps, "k": k, "dims": dims, "epochs": done, "arcs": int(ptr[-1]),
            "longest_row": int(deg.max()), "group": _umap.geometry(),
            "device_ms": {"knn": ms["knn"], "graph": ms["graph"], "epoch_mean": ms["epoch"], "run": ms["run"]},
            "timed_epochs": ms["n_timed"], "last_epoch": {"arcs_fired": fired, "samples": drawn},
            "arcs_fired_per_second": fired / (ms["epoch"] * 1e-3), "gathered_bytes_per_second": gathered / (ms["epoch"] * 1e-3),
            "position_table_bytes": n * dims * 8, "l2_resident_gather_upper_mark_TBs": list(L2_RESIDENT_GATHER_TBS),
            "run_wall_seconds": wall_run, "umap_fit_wall_seconds": wall_call, "finite": ok, "lib": _lib.so_digest()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--cells", type=int, nargs="*", default=None)
    ap.add_argument("--comps", type=int, default=50)
    ap.add_argument("--k", type=int, default=15)
    ap.add_argument("--epochs", type=int, default=200)
    ap.add_argument("--dims", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "umap_bench.jsonl"))
    a = ap.parse_args()
    cells = a.cells or ([20000] if a.quick else [100000, 1000000])
    for n in cells:
        r = bench(n, a.comps, a.k, a.epochs, a.dims)
        line = json.dumps(r)
        print(line, flush=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
