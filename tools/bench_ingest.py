#!/usr/bin/env python3
"""Benchmark of the Matrix Market reader (nabo_amd.MtxReader, include/nabo_ingest.h): 10x-shaped text synthesised in
memory, fed to the device in slices, both indexes fetched.

    python tools/bench_ingest.py [--entries 10000000 100000000] [--chunk-bytes 0] [--repeat 2] [--out profiles/ingest_bench.jsonl]
    /opt/conda/bin/python3.9 tools/bench_ingest.py --reference 100000        # the reference's mtx_to_h5 on the CPU (needs h5py, tqdm)

One JSON line per run: the text's size, the chunks, the device times between HIP events summed over the chunks (upload,
parse = parse kernel + scan of the tile counts + placement, sort, transpose, download), the rates they give -- parse and
upload in GB/s of TEXT -- and the whole call in seconds on the host clock (feed + finish + both downloads; the text is
already in memory, so no disk and no inflate).  Beside the figures stand the yardsticks: the host link's 63 GB/s
specification and the 6.29 TB/s measured for an HBM copy.  When the parse rate is below the upload rate of the same run,
the parser is the bottleneck of the device side, and the line says so.
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

N_GENES, PER_CELL = 32000, 2000     # a cell lists 2000 of 32000 genes: one in every stride of 16
POW10 = 10 ** np.arange(1, 19, dtype=np.int64)
HOST_LINK_GBPS, HBM_COPY_TBPS = 63.0, 6.29


def render(cols, seps):
    """the lines `c0 sep0 c1 sep1 ...` of non-negative int64 columns as one uint8 array, digits as %d prints them"""
    n = cols[0].shape[0]
    widths = [np.searchsorted(POW10, c, side="right").astype(np.int64) + 1 for c in cols]
    start = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(sum(widths) + len(cols), out=start[1:])
    out = np.empty(int(start[-1]), dtype=np.uint8)
    pos = start[:-1].copy()
    for c, w, sep in zip(cols, widths, seps):
        end = pos + w
        out[end] = sep
        rem, idx = c.copy(), np.arange(n)
        for k in range(1, int(w.max()) + 1):
            idx = idx[w[idx] >= k]
            out[end[idx] - k] = 48 + rem[idx] % 10
            rem //= 10
        pos = end + 1
    return out


def synth(n_entries, seed=1, block=10 ** 7):
    """(text uint8, n_genes, n_cells): by cell, genes ascending inside a cell, counts mostly 1 .. 9 with a long tail"""
    rng = np.random.default_rng(seed)
    n_cells = (n_entries + PER_CELL - 1) // PER_CELL
    stride = N_GENES // PER_CELL
    parts = [np.frombuffer(b"%%%%MatrixMarket matrix coordinate integer general\n%%\n%d %d %d\n" % (N_GENES, n_cells, n_entries), dtype=np.uint8)]
    for at in range(0, n_entries, block):
        e = np.arange(at, min(at + block, n_entries), dtype=np.int64)
        gene = (e % PER_CELL) * stride + rng.integers(0, stride, size=e.shape[0]) + 1
        val = np.minimum(rng.geometric(0.35, size=e.shape[0]), 10 ** 6).astype(np.int64)
        parts.append(render([gene, e // PER_CELL + 1, val], [32, 32, 10]))
    return np.concatenate(parts), N_GENES, n_cells


def run(text, n_entries, chunk_bytes, feed_bytes):
    import nabo_amd
    t0 = time.perf_counter()
    with nabo_amd.MtxReader(chunk_bytes=chunk_bytes) as r:
        for at in range(0, text.shape[0], feed_bytes):
            r.feed(text[at:at + feed_bytes])
        m = r.finish()
        whole = time.perf_counter() - t0
        ms, chunks = r.last_device_ms()
    assert m.nnz == n_entries and int(m.cell_ptr[-1]) == n_entries and int(m.gene_ptr[-1]) == n_entries
    gb = text.shape[0] / 1e9
    rec = {"entries": n_entries, "text_bytes": int(text.shape[0]), "chunk_bytes": chunk_bytes, "chunks": chunks, "whole_call_s": round(whole, 4)}
    rec.update({k + "_ms": round(v, 3) for k, v in ms.items()})
    rec["parse_text_GBps"] = round(gb / (ms["parse"] / 1e3), 2)
    rec["upload_text_GBps"] = round(gb / (ms["upload"] / 1e3), 2)
    rec["whole_call_text_GBps"] = round(gb / whole, 3)
    rec["yardsticks"] = {"host_link_spec_GBps": HOST_LINK_GBPS, "hbm_copy_measured_TBps": HBM_COPY_TBPS}
    rec["device_side_bottleneck"] = "parser" if rec["parse_text_GBps"] < rec["upload_text_GBps"] else "upload"
    return rec


def reference(n_entries, ref_root):
    """seconds of the reference's mtx_to_h5 on a directory of n_entries, on the CPU"""
    import importlib.util
    import tempfile
    spec = importlib.util.spec_from_file_location("nabo_ref_io", os.path.join(ref_root, "nabo", "_io.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    text, n_genes, n_cells = synth(n_entries)
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "matrix.mtx"), "wb") as f:
            f.write(text.tobytes())
        with open(os.path.join(d, "genes.tsv"), "w") as f:
            f.write("".join("ID%d\tG%d\n" % (g, g) for g in range(n_genes)))
        with open(os.path.join(d, "barcodes.tsv"), "w") as f:
            f.write("".join("C%d\n" % c for c in range(n_cells)))
        t0 = time.perf_counter()
        mod.mtx_to_h5(d, os.path.join(d, "out.h5"))
        return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entries", type=int, nargs="+", default=[10 ** 7, 10 ** 8])
    ap.add_argument("--chunk-bytes", type=int, default=0)
    ap.add_argument("--feed-bytes", type=int, default=64 << 20)
    ap.add_argument("--repeat", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "ingest_bench.jsonl"))
    ap.add_argument("--reference", type=int, default=0, help="time the reference's mtx_to_h5 on this many entries instead")
    ap.add_argument("--reference-root", default=os.environ.get("NABO_REFERENCE", "/root/reference"))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as out:
        if a.reference:
            rec = {"reference_mtx_to_h5": True, "entries": a.reference, "seconds_cpu": round(reference(a.reference, a.reference_root), 3)}
            print(json.dumps(rec), flush=True)
            out.write(json.dumps(rec) + "\n")
            return
        for n in a.entries:
            t0 = time.perf_counter()
            text, _, _ = synth(n)
            print("# %d entries: %.2f GB of text synthesised in %.1f s" % (n, text.shape[0] / 1e9, time.perf_counter() - t0), flush=True)
            for rep in range(a.repeat):
                rec = run(text, n, a.chunk_bytes, a.feed_bytes)
                rec["repeat"] = rep
                print(json.dumps(rec), flush=True)
                out.write(json.dumps(rec) + "\n")
                out.flush()


if __name__ == "__main__":
    main()
