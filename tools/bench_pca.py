#!/usr/bin/env python3
"""Times the PCA projection of sparse cells and the gene statistics on the GPU at a stated size, and -- separately, on a
CPU -- the reference's per-cell loop on a stated sub-sample.  No pass / fail threshold: the step has no earlier version
in this project to compare with.

    python tools/bench_pca.py [--quick] [--cells 1000000] [--raw-genes 20000] [--density 0.05] [--genes 2000] [--comps 50]
        nabo_pca_project over all cells in the library's default chunks, then nabo_gene_stats over all raw genes.  Prints
        one JSON line: whole-call seconds (median of the repeats after one warm-up; host validation, staging, uploads,
        kernels, downloads), device ms per phase from nabo_pca_last_device_ms, chunks, and two rates of the projection
        kernel: the bytes of component-table rows it gathers per second -- to be read against the 16.8-18.8 TB/s the
        MI355X serves chip-wide for rows gathered from a table resident in L2 -- and the bytes of CSR it streams from HBM
        per second.  --quick: 100 000 cells x 5 000 raw genes, 1 000 selected.

    python3.9 tools/bench_pca.py --reference /path/to/nabo-checkout [--cells 3000] [--raw-genes 2000] [--genes 500]
        the reference's set_gene_stats, and its transform_pca loop, on a dataset of that size written to a temporary
        HDF5 file (needs h5py, pandas, sklearn).  Both loops grow linearly with the cells (genes).
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


def synth_csr(n_cells, n_raw, density, seed=11, block=50000):
    """per cell one candidate gene in each of n_raw * density / 0.9 equal strides (strictly increasing), a tenth of them
    dropped again; built in blocks of cells to bound the temporaries"""
    rng = np.random.default_rng(seed)
    per_cell = max(1, int(round(n_raw * density / 0.9)))
    stride = n_raw // per_cell
    base = (np.arange(per_cell, dtype=np.int32) * stride)[None, :]
    counts, genes = [], []
    for c0 in range(0, n_cells, block):
        n = min(block, n_cells - c0)
        g = base + rng.integers(0, stride, (n, per_cell), dtype=np.int32)
        keep = rng.random((n, per_cell), dtype=np.float32) < 0.9
        counts.append(keep.sum(axis=1))
        genes.append(g[keep])
    gene = np.concatenate(genes)
    cell_ptr = np.concatenate([[0], np.cumsum(np.concatenate(counts))]).astype(np.int64)
    val = (rng.poisson(1.5, gene.shape[0]) + 1).astype(np.float32)
    sf = (0.5 + rng.random(n_cells)).astype(np.float32)
    return cell_ptr, gene, val, sf


def tables(n_raw, n_sel, n_comps, seed=12):
    rng = np.random.default_rng(seed)
    gene_pos = np.full(n_raw, -1, dtype=np.int32)
    gene_pos[np.sort(rng.permutation(n_raw)[:n_sel])] = rng.permutation(n_sel)
    return gene_pos, rng.random(n_sel), 0.5 + rng.random(n_sel), rng.normal(size=n_sel) * 0.1, rng.normal(size=(n_comps, n_sel)) / np.sqrt(n_sel)


def run_gpu(a):
    from nabo_amd import _matrixio, _pca
    m = _matrixio.csr(synth_csr(a.cells, a.raw_genes, a.density))
    t = _pca._tables(*tables(a.raw_genes, a.genes, a.comps))
    nnz = int(m[1][-1])
    selected = int((t[0][m[2]] >= 0).sum())
    secs, ms, chunks = [], None, 0
    for r in range(a.repeats + 1):
        t0 = time.perf_counter()
        _pca._device_project(m, *t, None, mem_budget=a.budget)
        if r:
            secs.append(time.perf_counter() - t0)
        ms, chunks = _pca.last_device_ms()
    gathered, streamed = selected * a.comps * 8, nnz * 8 + a.cells * 12
    out = {"bench": "pca_project", "cells": a.cells, "raw_genes": a.raw_genes, "selected_genes": a.genes, "comps": a.comps, "nnz": nnz,
           "density": nnz / (a.cells * a.raw_genes), "selected_entries": selected, "seconds": statistics.median(secs), "seconds_all": secs,
           "device_ms": ms, "chunks": chunks, "table_bytes": a.genes * a.comps * 8,
           "gathered_TB_per_s": gathered / (ms["kernel"] * 1e-3) / 1e12, "gather_roofline_TB_per_s": [16.8, 18.8],
           "csr_streamed_GB_per_s": streamed / (ms["kernel"] * 1e-3) / 1e9, "z_written_GB_per_s": a.cells * a.comps * 8 / (ms["kernel"] * 1e-3) / 1e9}
    print(json.dumps(out), flush=True)
    # ---- the gene statistics of every raw gene
    cell = np.repeat(np.arange(a.cells, dtype=np.int32), np.diff(m[1]))
    order = np.argsort(m[2], kind="stable")
    gene_ptr = np.concatenate([[0], np.cumsum(np.bincount(m[2], minlength=a.raw_genes))]).astype(np.int64)
    csc = _matrixio.csc((gene_ptr, cell[order], m[3][order], m[4]), "bench")
    del cell, order
    secs = []
    for r in range(a.repeats + 1):
        t0 = time.perf_counter()
        _pca._device_stats(csc, None, None)
        if r:
            secs.append(time.perf_counter() - t0)
        ms, chunks = _pca.last_device_ms()
    print(json.dumps({"bench": "gene_stats", "cells": a.cells, "genes": a.raw_genes, "nnz": nnz, "seconds": statistics.median(secs), "seconds_all": secs,
                      "device_ms": ms, "chunks": chunks, "csc_read_twice_GB_per_s": 2 * nnz * 8 / (ms["kernel"] * 1e-3) / 1e9}))


def run_reference(a):
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import gen_golden_pca as gg
    gg.REF = a.reference
    ds_mod = gg.load_reference()
    rng = np.random.default_rng(3)
    X = gg.synth(rng, a.cells, a.raw_genes, a.density / 3)      # (its density grows with j % 5: about the asked one on average)
    cells, genes = ["c%d" % i for i in range(a.cells)], ["G%d" % j for j in range(a.raw_genes)]
    sf = (0.5 + rng.random(a.cells)).astype(np.float32)
    with tempfile.TemporaryDirectory() as td:
        fn = os.path.join(td, "bench.h5")
        gg.write_dataset(fn, cells, genes, X, sf, None, None)
        ds = gg.quiet(ds_mod.Dataset, fn)
        t0 = time.perf_counter()
        gg.quiet(ds.set_gene_stats)
        s_stats = time.perf_counter() - t0
        sel = list(gg.quiet(ds.get_scaling_params).index[:a.genes])
        gg.quiet(ds.fit_ipca, sel, a.comps, None, True)
        sp = gg.quiet(ds.get_scaling_params, sel)
        t0 = time.perf_counter()
        gg.quiet(ds.transform_pca, os.path.join(td, "out.h5"), "pca", ds.ipca, sp, True)
        s_proj = time.perf_counter() - t0
    print(json.dumps({"bench": "reference set_gene_stats + transform_pca (CPU)", "cells": a.cells, "raw_genes": a.raw_genes, "selected_genes": len(sel),
                      "comps": a.comps, "nnz": int((X != 0).sum()), "set_gene_stats_seconds": s_stats, "transform_pca_seconds": s_proj}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--cells", type=int, default=None)
    ap.add_argument("--raw-genes", type=int, default=None)
    ap.add_argument("--density", type=float, default=0.05)
    ap.add_argument("--genes", type=int, default=None, help="selected genes")
    ap.add_argument("--comps", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--budget", type=int, default=0, help="device-memory budget of the row chunks in bytes (0: the library's default)")
    ap.add_argument("--reference", default=None, help="a checkout of the reference: time IT on the CPU instead")
    a = ap.parse_args()
    small = a.reference is not None
    a.cells = a.cells or (3000 if small else 100000 if a.quick else 1000000)
    a.raw_genes = a.raw_genes or (2000 if small else 5000 if a.quick else 20000)
    a.genes = a.genes or (500 if small else 1000 if a.quick else 2000)
    return run_reference(a) if small else run_gpu(a)


if __name__ == "__main__":
    sys.exit(main())
