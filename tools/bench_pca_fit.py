#!/usr/bin/env python3
"""Times the exact PCA fit on the GPU at a stated size, and -- separately, on a CPU -- sklearn's IncrementalPCA with the
reference's batching (Dataset.fit_ipca) at a stated smaller size.  No pass / fail threshold: the kernel has no earlier
version in this project to compare with.

    python tools/bench_pca_fit.py [--quick] [--cells 1000000] [--raw-genes 20000] [--density 0.05] [--genes 2000] [--comps 100]
        fit_pca_csr over all cells in the library's default chunks.  Prints one JSON line per run: device ms per phase
        (nabo_pca_cov_last_phase_ms) and as uploads / kernels / downloads (nabo_pca_last_device_ms), chunks, the
        whole-call seconds with the host eigen-solve as its own field and share, and the float64 flop/s of the product
        phase counted as n G^2 (the half of the symmetric result that is computed), beside the peak it is divided by:
        78.6 Tflop/s, the FP64 matrix peak of AMD's public MI355X data sheet.  --quick: 100 000 cells x 5 000 raw genes,
        1 000 selected.

    python3.9 tools/bench_pca_fit.py --reference [--cells 20000] [--genes 1000] [--comps 100]
        sklearn's IncrementalPCA.partial_fit over dense scaled cells in the reference's batches (2 * n_comps cells,
        evened out as its make_eq_bins does), on the CPU, without the reference's per-cell HDF5 reads and Python
        densifying, which only add to it.  Needs sklearn.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
from bench_pca import synth_csr  # noqa: E402

FP64_MATRIX_PEAK = 78.6e12
PEAK_SOURCE = "AMD Instinct MI355X data sheet, peak FP64 matrix"


def run_gpu(a):
    from nabo_amd import _matrixio, _pca
    m = _matrixio.csr(synth_csr(a.cells, a.raw_genes, a.density))
    rng = np.random.default_rng(12)
    gene_pos = np.full(a.raw_genes, -1, dtype=np.int32)
    gene_pos[np.sort(rng.permutation(a.raw_genes)[:a.genes])] = rng.permutation(a.genes)
    t = _pca._fit_tables(gene_pos, 0.2 * rng.random(a.genes), 0.5 + rng.random(a.genes))
    for r in range(a.repeats + 1):
        t0 = time.perf_counter()
        mean, cov = _pca._device_cov(m, *t, None, mem_budget=a.budget)
        t1 = time.perf_counter()
        _pca.FittedPCA(mean, cov, a.cells, a.comps)
        t2 = time.perf_counter()
        if not r:
            continue                                            # the warm-up
        (ms, chunks), phase = _pca.last_device_ms(), _pca.last_cov_phase_ms()
        flops = a.cells * a.genes ** 2 / (phase["product"] * 1e-3)
        print(json.dumps({"bench": "pca_fit", "cells": a.cells, "raw_genes": a.raw_genes, "selected_genes": a.genes, "comps": a.comps,
                          "nnz": int(m[1][-1]), "density": int(m[1][-1]) / (a.cells * a.raw_genes), "chunks": chunks, "phase_ms": phase,
                          "device_ms": ms, "seconds": t2 - t0, "cov_call_seconds": t1 - t0, "host_eigh_seconds": t2 - t1,
                          "host_eigh_share": (t2 - t1) / (t2 - t0), "product_flop": a.cells * a.genes ** 2, "product_flop_per_s": flops,
                          "fp64_matrix_peak_flop_per_s": FP64_MATRIX_PEAK, "peak_source": PEAK_SOURCE, "product_share_of_peak": flops / FP64_MATRIX_PEAK}),
              flush=True)


def run_reference(a):
    from sklearn.decomposition import IncrementalPCA
    rng = np.random.default_rng(3)
    Y = np.where(rng.random((a.cells, a.genes)) < a.density, rng.poisson(1.5, (a.cells, a.genes)) + 1.0, 0.0)
    Y = (Y - Y.mean(axis=0)) / Y.std(axis=0)
    bs = min(2 * a.comps, a.cells)
    n_bins = a.cells // bs
    sizes = [a.cells // n_bins + (1 if i < a.cells % n_bins else 0) for i in range(n_bins)]
    secs = []
    for r in range(a.repeats):
        ipca = IncrementalPCA(n_components=a.comps)
        t0, r0 = time.perf_counter(), 0
        for s in sizes:
            ipca.partial_fit(Y[r0:r0 + s])
            r0 += s
        secs.append(time.perf_counter() - t0)
    print(json.dumps({"bench": "sklearn IncrementalPCA in the reference's batches (CPU)", "cells": a.cells, "selected_genes": a.genes,
                      "comps": a.comps, "batches": n_bins, "batch_size": sizes[0], "threads": os.cpu_count(), "seconds": statistics.median(secs),
                      "seconds_all": secs}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--cells", type=int, default=None)
    ap.add_argument("--raw-genes", type=int, default=None)
    ap.add_argument("--density", type=float, default=0.05)
    ap.add_argument("--genes", type=int, default=None, help="selected genes")
    ap.add_argument("--comps", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--budget", type=int, default=0, help="device-memory budget in bytes (0: the library's default)")
    ap.add_argument("--reference", action="store_true", help="time sklearn's IncrementalPCA on the CPU instead")
    a = ap.parse_args()
    a.cells = a.cells or (20000 if a.reference else 100000 if a.quick else 1000000)
    a.raw_genes = a.raw_genes or (5000 if a.quick else 20000)
    a.genes = a.genes or (1000 if a.reference or a.quick else 2000)
    return run_reference(a) if a.reference else run_gpu(a)


if __name__ == "__main__":
    sys.exit(main())
