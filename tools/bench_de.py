#!/usr/bin/env python3
"""Times find_cluster_markers' work on the GPU at a stated size, and -- separately, on a CPU -- the reference on a stated
sub-sample.  No pass / fail threshold: the step has no earlier version in this project to compare with.

    python tools/bench_de.py [--cells 200000] [--genes 2000] [--clusters 16] [--repeats 3]
        every cluster against every other in one device call (nabo_amd._de._markers_from_csc on arrays: planning, uploads,
        kernels, the exact p-values, the tables; reading the HDF5 file is left out).  Prints one JSON line: whole-call
        seconds (median of the repeats after one warm-up), device ms per phase from nabo_de_last_device_ms, gene chunks.

    python3.9 tools/bench_de.py --reference /path/to/nabo-checkout [--cells 3000] [--genes 400] [--clusters 4]
        the reference's find_cluster_markers on a dataset of that size written to a temporary HDF5 file (needs h5py,
        pandas, scipy >= 1.7, statsmodels).  Its loop grows with cells x genes x clusters^2.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)


def synth(n_cells, n_genes, n_clusters, seed=7):
    """single-cell-like sparsity: every gene in 4 % of the cells, every fourth gene in 40 % of its home cluster with
    doubled counts; (cells, columns [(idx, val)], size factors, cluster of every cell)"""
    rng = np.random.default_rng(seed)
    cluster = rng.integers(0, n_clusters, n_cells)
    sf = (0.5 + rng.random(n_cells)).astype(np.float32)
    cols = []
    for j in range(n_genes):
        p = np.full(n_cells, 0.04)
        home = cluster == j % n_clusters
        if j % 4 == 0:
            p[home] = 0.4
        idx = np.nonzero(rng.random(n_cells) < p)[0]
        lam = np.where(home[idx], 3.0, 1.5) if j % 4 == 0 else 1.5
        cols.append((idx.astype(np.int32), (rng.poisson(lam, idx.shape[0]) + 1).astype(np.float32)))
    return cols, sf, cluster


def run_gpu(a):
    from nabo_amd import _de, _matrixio
    cols, sf, cluster = synth(a.cells, a.genes, a.clusters)
    ptr = np.concatenate([[0], np.cumsum([len(i) for i, _ in cols])]).astype(np.int64)
    m = _matrixio.csc((ptr, np.concatenate([i for i, _ in cols]), np.concatenate([v for _, v in cols]), sf), "bench")
    genes = ["G%d" % j for j in range(a.genes)]
    clusters = {"c%d_S" % i: int(c) + 1 for i, c in enumerate(cluster)}
    cell_idx = {"c%d" % i: i for i in range(a.cells)}

    def step(*args):
        return _de._device_de(*args, mem_budget=a.budget)
    secs, ms, rows = [], None, 0
    for r in range(a.repeats + 1):
        t = time.perf_counter()
        table, de_genes = _de._markers_from_csc(clusters, genes, m, a.clusters // 2, 0.25, 0.5, 0.05, cell_idx, step)
        if r:
            secs.append(time.perf_counter() - t)
        ms, chunks = _de.last_device_ms()
        rows = len(table["gene"])
    print(json.dumps({"bench": "find_cluster_markers", "cells": a.cells, "genes": a.genes, "clusters": a.clusters, "nnz": int(ptr[-1]),
                      "pairs_per_gene": a.clusters * (a.clusters - 1), "seconds": statistics.median(secs), "seconds_all": secs,
                      "device_ms": ms, "chunks": chunks, "rows": rows, "marker_genes": sum(len(v) for v in de_genes.values())}))


def run_reference(a):
    import contextlib
    import io
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import gen_golden_de as gg
    gg.REF = a.reference
    ds_mod, mk = gg.load_reference()
    cols, sf, cluster = synth(a.cells, a.genes, a.clusters)
    cells, genes = ["c%d" % i for i in range(a.cells)], ["G%d" % j for j in range(a.genes)]
    with tempfile.TemporaryDirectory() as td:
        fn = os.path.join(td, "bench.h5")
        gg.write_dataset(fn, cells, genes, cols, sf, None)
        ds = gg.quiet(ds_mod.Dataset, fn)
        clusters = {"c%d_S" % i: int(c) + 1 for i, c in enumerate(cluster)}
        t = time.perf_counter()
        with contextlib.redirect_stderr(io.StringIO()):
            df, _ = mk.find_cluster_markers(clusters, ds, a.clusters // 2, exp_frac_thresh=0.25, log2_fc_thresh=0.5, qval_thresh=0.05)
        s = time.perf_counter() - t
    print(json.dumps({"bench": "reference find_cluster_markers (CPU)", "cells": a.cells, "genes": a.genes, "clusters": a.clusters,
                      "seconds": s, "rows": int(df.shape[0])}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=None)
    ap.add_argument("--genes", type=int, default=None)
    ap.add_argument("--clusters", type=int, default=None)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--budget", type=int, default=0, help="device-memory budget of the gene chunks in bytes (0: the library's default)")
    ap.add_argument("--reference", default=None, help="a checkout of the reference: time IT on the CPU instead")
    a = ap.parse_args()
    small = a.reference is not None
    a.cells = a.cells or (3000 if small else 200000)
    a.genes = a.genes or (400 if small else 2000)
    a.clusters = a.clusters or (4 if small else 16)
    return run_reference(a) if small else run_gpu(a)


if __name__ == "__main__":
    sys.exit(main())
