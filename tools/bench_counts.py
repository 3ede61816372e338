#!/usr/bin/env python3
"""Benchmark of the Matrix Market writer and of the remap of count matrices (nabo_amd.MtxWriter, remap_counts;
include/nabo_counts.h): a 10x-shaped cell index synthesised in memory, written as text into a host buffer, then cut to a
third of its cells and renumbered through a shuffled gene map with both indexes rebuilt.

    python tools/bench_counts.py [--entries 10000000 100000000] [--chunk-bytes 0] [--repeat 2] [--out profiles/counts_bench.jsonl]
    /opt/conda/bin/python3.9 tools/bench_counts.py --reference 100000       # the reference's three functions on the CPU (needs h5py, pandas, tqdm)

One JSON line per run.  Writer: the text's size, the chunks, the device times between HIP events (upload of the matrix,
lengths = length pass + scan, format and download summed over the chunks), the rates they give -- format and download in
GB/s of TEXT -- and the whole call in seconds on the host clock (create + every read into one host buffer; no disk).
Beside the figures stand the yardsticks already recorded for the reader (profiles/ingest_bench.jsonl): its parse at
157 GB/s of text and the 56 GB/s the host link gave its upload.  When the format rate is below the download rate of the
same run the formatter is the bottleneck of the device side, and the line says so.  Remap: the whole call on the host
clock (upload, kernels, sorts, both downloads) for a subset with the sort skipped and for a shuffled map with the sort.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)

N_GENES, PER_CELL = 32000, 2000     # a cell lists 2000 of 32000 genes: one in every stride of 16 (as tools/bench_ingest.py)
READER_PARSE_GBPS, HOST_LINK_MEASURED_GBPS = 157.0, 56.0


def synth(n_entries, seed=1):
    """(cell_ptr, gene, val, n_genes): genes ascending inside a cell, counts mostly 1 .. 9 with a long tail"""
    rng = np.random.default_rng(seed)
    n_cells = (n_entries + PER_CELL - 1) // PER_CELL
    stride = N_GENES // PER_CELL
    e = np.arange(n_entries, dtype=np.int64)
    gene = ((e % PER_CELL) * stride + rng.integers(0, stride, size=n_entries)).astype(np.int32)
    val = np.minimum(rng.geometric(0.35, size=n_entries), 10 ** 6).astype(np.uint32)
    ptr = np.minimum(np.arange(n_cells + 1, dtype=np.int64) * PER_CELL, n_entries)
    return ptr, gene, val, N_GENES


def run_writer(m, n_genes, chunk_bytes):
    import nabo_amd
    t0 = time.perf_counter()
    with nabo_amd.MtxWriter(m, n_genes, chunk_bytes=chunk_bytes) as w:
        buf = np.empty(w.total_bytes, dtype=np.uint8)
        at = 0
        while at < w.total_bytes:
            n = w.readinto(buf[at:])
            assert n > 0
            at += n
        whole = time.perf_counter() - t0
        ms, chunks = w.last_device_ms()
    assert buf[-1] == 10 and int((buf[-200:] == 10).sum()) > 5
    gb = buf.shape[0] / 1e9
    rec = {"writer": True, "entries": int(m[1].shape[0]), "text_bytes": int(buf.shape[0]), "chunk_bytes": chunk_bytes, "chunks": chunks,
           "whole_call_s": round(whole, 4)}
    rec.update({k + "_ms": round(v, 3) for k, v in ms.items()})
    rec["format_text_GBps"] = round(gb / (ms["format"] / 1e3), 2)
    rec["download_text_GBps"] = round(gb / (ms["download"] / 1e3), 2)
    rec["whole_call_text_GBps"] = round(gb / whole, 3)
    rec["yardsticks"] = {"reader_parse_text_GBps": READER_PARSE_GBPS, "host_link_measured_GBps": HOST_LINK_MEASURED_GBPS}
    rec["device_side_bottleneck"] = "formatter" if rec["format_text_GBps"] < rec["download_text_GBps"] else "download"
    return rec


def run_remap(m, n_genes, kind, seed=3):
    import nabo_amd
    rng = np.random.default_rng(seed)
    n_cells = m[0].shape[0] - 1
    if kind == "subset":                                        # a third of the cells, all genes: the sort is skipped
        rows, col_map = np.sort(rng.permutation(n_cells)[:max(n_cells // 3, 1)]), np.arange(n_genes, dtype=np.int32)
    else:                                                       # every cell, the genes renumbered at random: sorted
        rows, col_map = np.arange(n_cells), rng.permutation(n_genes).astype(np.int32)
    t0 = time.perf_counter()
    csr, csc = nabo_amd.remap_counts(m[0], m[1], m[2], n_genes, rows, col_map, n_genes)
    whole = time.perf_counter() - t0
    assert csc[0][-1] == csr[0][-1] == len(csr[1])
    return {"remap": kind, "entries_in": int(m[1].shape[0]), "entries_out": int(len(csr[1])), "whole_call_s": round(whole, 4),
            "entries_out_per_s": round(len(csr[1]) / whole, 1)}


def reference(n_entries, ref_root):
    """seconds of the reference's h5_to_mtx, extract_cells_from_h5 (a third of the cells) and merge_h5 (the file with itself)
    on a dataset file of n_entries, on the CPU"""
    import contextlib
    import io
    import random
    import tempfile
    sys.path.insert(0, os.path.join(REPO, "tests"))
    sys.path.insert(0, HERE)
    import _counts_ref as cref
    import _ingest_ref as iref
    import gen_golden_counts
    gen_golden_counts.REF = ref_root
    ref = gen_golden_counts.load_reference()
    ptr, gene, val, n_genes = synth(n_entries)
    n_cells = ptr.shape[0] - 1
    cell = np.repeat(np.arange(n_cells), np.diff(ptr))
    csc = iref.index_by(gene.astype(np.int64), cell, val, n_genes)
    genes, cells = ["G%d" % g for g in range(n_genes)], ["C%d" % c for c in range(n_cells)]
    out, cwd = {}, os.getcwd()
    with tempfile.TemporaryDirectory() as d:
        fn = os.path.join(d, "in.h5")
        cref.write_dataset(fn, genes, cells, (ptr, gene, val), csc)
        os.makedirs(os.path.join(d, "mtx"))
        os.chdir(d)
        try:
            random.seed(1)
            for name, call in (("h5_to_mtx", lambda: ref.h5_to_mtx(fn, os.path.join(d, "mtx"))),
                               ("extract_cells_from_h5", lambda: ref.extract_cells_from_h5(fn, os.path.join(d, "ex.h5"), cells[::3])),
                               ("merge_h5", lambda: ref.merge_h5([fn, fn], os.path.join(d, "mg.h5")))):
                t0 = time.perf_counter()
                with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
                    call()
                out[name + "_seconds_cpu"] = round(time.perf_counter() - t0, 3)
        finally:
            os.chdir(cwd)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entries", type=int, nargs="+", default=[10 ** 7, 10 ** 8])
    ap.add_argument("--chunk-bytes", type=int, default=0)
    ap.add_argument("--repeat", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "counts_bench.jsonl"))
    ap.add_argument("--reference", type=int, default=0, help="time the reference's three functions on this many entries instead")
    ap.add_argument("--reference-root", default=os.environ.get("NABO_REFERENCE", "/root/reference"))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as out:
        def emit(rec):
            print(json.dumps(rec), flush=True)
            out.write(json.dumps(rec) + "\n")
            out.flush()
        if a.reference:
            rec = {"reference": True, "entries": a.reference}
            rec.update(reference(a.reference, a.reference_root))
            emit(rec)
            return
        for n in a.entries:
            ptr, gene, val, n_genes = synth(n)
            print("# %d entries in %d cells synthesised" % (n, ptr.shape[0] - 1), flush=True)
            for rep in range(a.repeat):
                for rec in (run_writer((ptr, gene, val), n_genes, a.chunk_bytes), run_remap((ptr, gene, val), n_genes, "subset"),
                            run_remap((ptr, gene, val), n_genes, "shuffled_genes")):
                    rec["repeat"] = rep
                    emit(rec)


if __name__ == "__main__":
    main()
