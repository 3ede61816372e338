#!/usr/bin/env python3
"""Benchmark of the CSV reader (nabo_amd.CsvReader, include/nabo_csv.h): a dense gene x cell table synthesised in memory,
fed to the device in slices, both indexes fetched.

    python tools/bench_csv.py [--quick] [--rows 20000] [--cols 10000] [--chunk-bytes 0] [--repeat 2] [--out profiles/csv_bench.jsonl]
    /opt/conda/bin/python3.9 tools/bench_csv.py --reference 200        # the reference's csv_to_h5 on the CPU (needs h5py, tqdm)

Two tables per run, 10 % of the fields non-zero: integer counts (`0` and small integers, about 2 bytes a field) and
17-digit values (`0` and repr of a double, as log-normalised data is written).  The table is a block of 500 distinct rows
repeated, with a row name in front of every line; the parser does not know.  One JSON line per table: the text's size, the
chunks, the device times between HIP events summed over the chunks (upload, parse = count + bases + conversion + placement
with the host's deferred fields in between, transpose = row_ptr + the by-column index, download), the parse and upload
rates in GB/s of TEXT, fields per second, the share of fields deferred to the host, and the whole call in seconds on the
host clock (feed + finish + both downloads; the text is already in memory).  Beside the figures stand the yardsticks, not
thresholds: the Matrix Market parser's recorded 157 GB/s of text and the 6.29 TB/s measured for an HBM copy.
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

BLOCK_ROWS, NONZERO = 500, 0.10
MTX_PARSE_GBPS, HBM_COPY_TBPS = 157.0, 6.29


def synth(n_rows, n_cols, kind, seed=1):
    """the body of the table as bytes: `g<i>,v,v,...` lines; kind "int": counts, "repr": 17-digit doubles"""
    rng = np.random.default_rng(seed)
    block = []
    for _ in range(min(BLOCK_ROWS, n_rows)):
        fields = [b"0"] * n_cols
        at = np.flatnonzero(rng.random(n_cols) < NONZERO)
        if kind == "int":
            vals = [b"%d" % v for v in rng.geometric(0.3, size=at.shape[0]).tolist()]
        else:
            vals = [repr(v).encode() for v in np.log2(1.0 + rng.gamma(2.0, 3.0, size=at.shape[0])).tolist()]
        for i, v in zip(at.tolist(), vals):
            fields[i] = v
        block.append(b"," + b",".join(fields) + b"\n")
    return b"".join(b"g%d" % r + block[r % len(block)] for r in range(n_rows))


def run(text, n_rows, n_cols, kind, chunk_bytes, feed_bytes):
    import nabo_amd
    view = np.frombuffer(text, dtype=np.uint8)
    t0 = time.perf_counter()
    with nabo_amd.CsvReader(",", n_cols, True, float if kind == "repr" else int, chunk_bytes=chunk_bytes) as r:
        for at in range(0, view.shape[0], feed_bytes):
            r.feed(view[at:at + feed_bytes])
        m = r.finish()
        whole = time.perf_counter() - t0
        ms, chunks = r.last_device_ms()
        stats = r.stats()
    assert m.n_rows == n_rows and stats["fields"] == n_rows * n_cols and int(m.row_ptr[-1]) == m.nnz == stats["entries"]
    gb = len(text) / 1e9
    rec = {"table": kind, "rows": n_rows, "cols": n_cols, "text_bytes": len(text), "nnz": m.nnz, "chunk_bytes": chunk_bytes, "chunks": chunks,
           "whole_call_s": round(whole, 4)}
    rec.update({k + "_ms": round(v, 3) for k, v in ms.items()})
    rec["parse_text_GBps"] = round(gb / (ms["parse"] / 1e3), 2)
    rec["upload_text_GBps"] = round(gb / (ms["upload"] / 1e3), 2)
    rec["parse_fields_per_s"] = round(stats["fields"] / (ms["parse"] / 1e3))
    rec["whole_call_text_GBps"] = round(gb / whole, 3)
    rec["deferred_share"] = stats["deferred"] / max(stats["fields"], 1)
    rec["yardsticks"] = {"mtx_parse_recorded_GBps": MTX_PARSE_GBPS, "hbm_copy_measured_TBps": HBM_COPY_TBPS}
    return rec


def reference(n_rows, n_cols, ref_root):
    """seconds of the reference's csv_to_h5 on a table of n_rows x n_cols integer counts, on the CPU"""
    import importlib.util
    import tempfile
    spec = importlib.util.spec_from_file_location("nabo_ref_io", os.path.join(ref_root, "nabo", "_io.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    head = (",".join(["gene"] + ["c%d" % c for c in range(n_cols)]) + "\n").encode()
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "t.csv"), "wb") as f:
            f.write(head + synth(n_rows, n_cols, "int"))
        t0 = time.perf_counter()
        mod.csv_to_h5(os.path.join(d, "t.csv"), os.path.join(d, "out.h5"))
        return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="2000 x 1000 instead of 20000 x 10000")
    ap.add_argument("--rows", type=int, default=20000)
    ap.add_argument("--cols", type=int, default=10000)
    ap.add_argument("--chunk-bytes", type=int, default=0)
    ap.add_argument("--feed-bytes", type=int, default=64 << 20)
    ap.add_argument("--repeat", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "csv_bench.jsonl"))
    ap.add_argument("--reference", type=int, default=0, help="time the reference's csv_to_h5 on this many rows of 1000 columns instead")
    ap.add_argument("--reference-root", default=os.environ.get("NABO_REFERENCE", "/root/reference"))
    a = ap.parse_args()
    if a.quick:
        a.rows, a.cols = 2000, 1000
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as out:
        if a.reference:
            rec = {"reference_csv_to_h5": True, "rows": a.reference, "cols": 1000, "seconds_cpu": round(reference(a.reference, 1000, a.reference_root), 3)}
            print(json.dumps(rec), flush=True)
            out.write(json.dumps(rec) + "\n")
            return
        for kind in ("int", "repr"):
            t0 = time.perf_counter()
            text = synth(a.rows, a.cols, kind)
            print("# %s: %d x %d, %.3f GB of text synthesised in %.1f s" % (kind, a.rows, a.cols, len(text) / 1e9, time.perf_counter() - t0), flush=True)
            for rep in range(a.repeat):
                rec = run(text, a.rows, a.cols, kind, a.chunk_bytes, a.feed_bytes)
                rec["repeat"] = rep
                print(json.dumps(rec), flush=True)
                out.write(json.dumps(rec) + "\n")
                out.flush()


if __name__ == "__main__":
    main()
