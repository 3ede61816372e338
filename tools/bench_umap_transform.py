#!/usr/bin/env python3
"""Times the UMAP transform (nabo_umap_transform_*: target cells placed in a reference embedding that does not move) on
the GPU.  Report only, no pass / fail threshold.

    python tools/bench_umap_transform.py [--quick] [--cells 100000 1000000] [--comps 50] [--k 15] [--epochs 100]

Reference and targets: nabo_amd._synth.pca_like (`--comps` components), `--cells` of each; --quick: 20 000.  The
reference positions are the first `--dims` components brought to [0, 10]: the timing needs positions, not a fit.  Per
case one JSON line, appended to profiles/umap_transform_bench.jsonl: device ms of the k-NN, of the graph build (parts B',
C' and the start of include/nabo_umap_transform.h) and of the ONE launch that runs every epoch; the attractive terms
and the negative samples of that run, and from them terms per second and gathered bytes per second (one position of
8 dims bytes per sample: the attraction reads registers); the wall time of the one call umap_transform.

The yardstick, not a threshold: the fit's epoch kernel reaches 1.1e10 terms per second at 1M cells
(profiles/umap_bench.jsonl: arcs fired plus samples of its last epoch over that epoch's time).  This loop carries no
schedule or position traffic per epoch.
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

FIT_EPOCH_TERMS_PER_SECOND = 1.1e10


def bench(n, comps, k, epochs, dims, seed=0):
    import nabo_amd
    from nabo_amd import _lib, _umap
    from nabo_amd._synth import pca_like
    cells = pca_like(2 * n, comps, seed=77)
    X, Z = np.ascontiguousarray(cells[0::2]), np.ascontiguousarray(cells[1::2])
    a, b = nabo_amd.find_ab_params(1.0, 0.1)
    Y = _umap.scale_start(X[:, :dims])
    with _umap.UmapTransform(n, dims, n_epochs=epochs, a=a, b=b, seed=seed) as T:
        T.set_embedding(Y).set_cells(X)
        T.query(Z, k)
        y0 = T.get_positions()
        T.run(2)                                   # warm-up: the first launch
        T.rewind().set_positions(y0)
        t0 = time.perf_counter()
        done = T.run()
        wall_run = time.perf_counter() - t0
        ms, c = T.last_ms(), T.last_run_counts()
        ok = bool(np.isfinite(T.get_positions()).all())
    fired, drawn = int(c["n_attr"].sum()), int(c["n_neg"].sum())
    t0 = time.perf_counter()
    nabo_amd.umap_transform(Z, X, Y, k, n_epochs=epochs, seed=seed)
    wall_call = time.perf_counter() - t0
    return {"bench": "umap_transform", "ref_cells": n, "targets": n, "comps": comps, "k": k, "dims": dims, "epochs": done,
            "group": _umap.transform_geometry(), "device_ms": {"knn": ms["knn"], "graph": ms["graph"], "run": ms["run"]},
            "run": {"attractive_terms": fired, "samples": drawn}, "terms_per_second": (fired + drawn) / (ms["run"] * 1e-3),
            "gathered_bytes_per_second": drawn * dims * 8 / (ms["run"] * 1e-3), "position_table_bytes": n * dims * 8,
            "fit_epoch_kernel_terms_per_second": FIT_EPOCH_TERMS_PER_SECOND, "run_wall_seconds": wall_run,
            "umap_transform_wall_seconds": wall_call, "finite": ok, "lib": _lib.so_digest()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--cells", type=int, nargs="*", default=None)
    ap.add_argument("--comps", type=int, default=50)
    ap.add_argument("--k", type=int, default=15)
    ap.add_argument("--epochs", type=int, default=100)
    ap.add_argument("--dims", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "umap_transform_bench.jsonl"))
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
