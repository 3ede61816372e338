#!/usr/bin/env python3
"""Times the per-cell quality-control pass on the GPU at a stated size, and -- separately, on a CPU -- the reference's
filter_data + set_sf on a stated small size.  No pass / fail threshold: the step has no earlier version in this project
to compare with.

    python tools/bench_qc.py [--quick] [--cells 1000000] [--raw-genes 20000] [--density 0.05] [--classes 3]
        nabo_cell_qc over all cells in the library's default chunks.  Prints one JSON line: whole-call seconds (median of
        the repeats after one warm-up; host validation, uploads, kernel, downloads), device ms per phase from
        nabo_qc_last_device_ms, chunks, and the bytes of CSR (8 per entry, 8 per row pointer) the kernel streams per
        second -- to be read against the 6.0-6.3 TB/s the MI355X sustains for HBM streamed in order.  A matrix below
        256 MiB (--quick: 100 000 cells x 5 000 raw genes, 200 MB) can sit in the Infinity Cache after its upload; the
        rate then says nothing about HBM.

    python3.9 tools/bench_qc.py --reference /path/to/nabo-checkout [--cells 3000] [--raw-genes 2000]
        the reference's filter_data and set_sf on a dataset of that size written to a temporary HDF5 file (needs h5py,
        pandas).  Both grow linearly with the cells.
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
sys.path.insert(0, os.path.join(REPO, "tools"))


def run_gpu(a):
    from bench_pca import synth_csr
    from nabo_amd import _matrixio, _qc
    cell_ptr, gene, val, _ = synth_csr(a.cells, a.raw_genes, a.density)
    m = _matrixio.csr((cell_ptr, gene, val))
    cls = np.random.default_rng(5).integers(0, 1 << max(a.classes, 1), a.raw_genes).astype(np.uint8)
    nnz = int(m[0][-1])
    secs, ms, chunks = [], None, 0
    for r in range(a.repeats + 1):
        t0 = time.perf_counter()
        _qc._device_qc(*m, cls, a.classes, mem_budget=a.budget)
        if r:
            secs.append(time.perf_counter() - t0)
        ms, chunks = _qc.last_device_ms()
    streamed = nnz * 8 + (a.cells + chunks) * 8
    print(json.dumps({"bench": "cell_qc", "cells": a.cells, "raw_genes": a.raw_genes, "classes": a.classes, "nnz": nnz,
                      "density": nnz / (a.cells * a.raw_genes), "class_table": "LDS" if a.raw_genes <= _qc.LDS_TABLE_GENES else "L2",
                      "seconds": statistics.median(secs), "seconds_all": secs, "device_ms": ms, "chunks": chunks, "csr_bytes": streamed,
                      "csr_streamed_TB_per_s": streamed / (ms["kernel"] * 1e-3) / 1e12, "hbm_stream_roofline_TB_per_s": [6.0, 6.3],
                      "fits_infinity_cache": streamed < 256 * 2 ** 20}), flush=True)


def run_reference(a):
    import gen_golden_pca as gg
    gg.REF = a.reference
    import types
    plot = types.ModuleType("nabo._plotting")
    plot.plot_mean_var = plot.plot_summary_data = lambda *x, **k: None
    sys.modules["nabo._plotting"] = plot
    ds_mod = gg.load_reference()
    rng = np.random.default_rng(3)
    X = gg.synth(rng, a.cells, a.raw_genes, a.density / 3)      # (its density grows with j % 5: about the asked one on average)
    cells, genes = ["c%d" % i for i in range(a.cells)], ["G%d" % j for j in range(a.raw_genes)]
    with tempfile.TemporaryDirectory() as td:
        fn = os.path.join(td, "bench.h5")
        gg.write_dataset(fn, cells, genes, X, np.ones(a.cells, np.float32), None, None)
        ds = gg.quiet(ds_mod.Dataset, fn)
        t0 = time.perf_counter()
        gg.quiet(ds.filter_data, min_exp=10, min_ngenes=5)
        s_filter = time.perf_counter() - t0
        t0 = time.perf_counter()
        gg.quiet(ds.set_sf)
        s_sf = time.perf_counter() - t0
    print(json.dumps({"bench": "reference filter_data + set_sf (CPU)", "cells": a.cells, "raw_genes": a.raw_genes, "nnz": int((X != 0).sum()),
                      "filter_data_seconds": s_filter, "set_sf_seconds": s_sf}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--cells", type=int, default=None)
    ap.add_argument("--raw-genes", type=int, default=None)
    ap.add_argument("--density", type=float, default=0.05)
    ap.add_argument("--classes", type=int, default=3, help="gene classes summed beside the total (0..8)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--budget", type=int, default=0, help="device-memory budget of the row chunks in bytes (0: the library's default)")
    ap.add_argument("--reference", default=None, help="a checkout of the reference: time IT on the CPU instead")
    a = ap.parse_args()
    small = a.reference is not None
    a.cells = a.cells or (3000 if small else 100000 if a.quick else 1000000)
    a.raw_genes = a.raw_genes or (2000 if small else 5000 if a.quick else 20000)
    return run_reference(a) if small else run_gpu(a)


if __name__ == "__main__":
    sys.exit(main())
