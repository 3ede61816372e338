#!/opt/conda/bin/python3.9
"""Golden vectors for the CSV reader: what the reference's csv_to_h5 (nabo/_io.py:238-477) writes.

TEST INFRASTRUCTURE ONLY, run where the reference is mounted, with an interpreter that has h5py, numpy and tqdm:

    /opt/conda/bin/python3.9 tools/gen_golden_csv.py

The reference's nabo/_io.py is loaded BY FILE PATH (it imports nothing of its package).  Three seeded tables of about
60 x 80 are written into a temporary directory, the reference's own csv_to_h5 runs on them, and only DATA goes to
tests/golden/csv.npz: the BYTES of the input files, the keyword arguments, and from the file the reference wrote the
names, the concatenated cell_data and gene_data records, their lengths and their dtypes.

A: integer counts, genes in rows, a header with quoted mixed-case names, two duplicated gene names, about 85 % zeros, an
   all-zero gene and an all-zero cell.
B: log-normalised values written with repr (17 digits), tab-separated, genes_in_columns=True, null_thresh, inv_log=2,
   rownames given and no name column.  The reference runs twice on it, with and without inv_log: `2 ** val` is numpy's
   power, which differs by an ulp between numpy builds, so the values in front of it are recorded as well (`_raw`).
C: value_dtype=int, with counts above 2^32.

Asserted, so that the tests can demand equality: the plain restatement (tests/_csv_ref.py) reproduces every record and
every name the reference wrote; and for sample B the restatement DEFERS NO FIELD -- a file of full-precision reprs is
converted by the device's rule, none of it handed back to the host.
"""
import contextlib
import importlib.util
import io
import json
import os
import sys
import tempfile

import h5py
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
REF = os.environ.get("NABO_REFERENCE", "/root/reference")
GOLD = os.path.join(REPO, "tests", "golden")
sys.path.insert(0, os.path.join(REPO, "tests"))
import _csv_ref as cref  # noqa: E402

N_GENES, N_CELLS = 60, 80


def load_reference():
    spec = importlib.util.spec_from_file_location("nabo_ref_io", os.path.join(REF, "nabo", "_io.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def counts(rng, zero_row, zero_col, big=None):
    m = rng.integers(1, 40, size=(N_GENES, N_CELLS)) * (rng.random((N_GENES, N_CELLS)) < 0.15)
    m[zero_row, :] = 0
    m[:, zero_col] = 0
    if big is not None:
        m[3, 5] = big
    return m


def sample_a():
    rng = np.random.default_rng(20250301)
    m = counts(rng, 17, 33)
    genes = ["Gene%d" % g for g in range(N_GENES)]
    genes[8], genes[21], genes[40] = "Dup", "dup", "DUP"        # one name three times, one twice: the reference's own scheme
    genes[50], genes[51] = "Xy", "xY"
    cells = ["Cell_%c%d" % ("ab"[c % 2], c) for c in range(N_CELLS)]
    head = ",".join(['"gene"'] + ['"%s"' % c for c in cells])
    lines = [",".join(["'%s'" % g if i % 2 else '"%s"' % g] + ["%d" % v for v in row]) for i, (g, row) in enumerate(zip(genes, m.tolist()))]
    return ("\n".join([head] + lines) + "\n").encode(), {}


def sample_b():
    rng = np.random.default_rng(20250302)
    m = counts(rng, 11, 44).T                                   # cells in rows
    v = np.log2(1.0 + m * rng.uniform(0.2, 3.0, size=m.shape))
    genes = ["g%d" % g for g in range(N_GENES)]
    head = "\t".join(genes)
    lines = ["\t".join(repr(float(x)) for x in row) for row in v]
    kw = dict(sep="\t", genes_in_columns=True, null_thresh=0.9, inv_log=2, rownames=["bc%d" % c for c in range(N_CELLS)])
    return ("\n".join([head] + lines) + "\n").encode(), kw


def sample_c():
    rng = np.random.default_rng(20250303)
    m = counts(rng, 2, 71, big=2 ** 40 + 7)
    genes = ["G%d" % g for g in range(N_GENES)]
    cells = ["c%d" % c for c in range(N_CELLS)]
    lines = [",".join([g] + ["%d" % x for x in row]) for g, row in zip(genes, m.tolist())]
    return ("\n".join([",".join(["id"] + cells)] + lines) + "\n").encode(), dict(value_dtype="int")


def flat(records):
    return (np.array([len(r) for r in records], dtype=np.int64), np.concatenate([r["idx"] for r in records]),
            np.concatenate([r["val"] for r in records]))


def main():
    ref = load_reference()
    out, meta = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        for s, make in (("A", sample_a), ("B", sample_b), ("C", sample_c)):
            data, kw = make()
            csv_fn, h5_fn = os.path.join(tmp, s + ".csv"), os.path.join(tmp, s + ".h5")
            with open(csv_fn, "wb") as f:
                f.write(data)
            ref_kw = dict(kw)
            if "value_dtype" in ref_kw:
                ref_kw["value_dtype"] = int
            with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
                ref.csv_to_h5(csv_fn, h5_fn, **ref_kw)
            with h5py.File(h5_fn, "r") as h5:
                genes = [x.decode() for x in h5["names"]["genes"][:]]
                cells = [x.decode() for x in h5["names"]["cells"][:]]
                cell_rec = [h5["cell_data"][c][:] for c in cells]
                gene_rec = [h5["gene_data"][g][:] for g in genes]
            dtypes = sorted({str(r.dtype) for r in cell_rec + gene_rec})
            assert len(dtypes) == 1, dtypes
            # the restatement reproduces all of it
            kind = 1 if kw.get("value_dtype") == "int" else 0
            by_row, by_col, rows, cols = cref.read_table(data, kw.get("sep", ","), kw.get("genes_in_columns", False), kw.get("inv_log"), kind,
                                                         kw.get("null_thresh"), kw.get("rownames"))
            in_cols = kw.get("genes_in_columns", False)
            assert (genes, cells) == ((cols, rows) if in_cols else (rows, cols)), s
            for records, (ptr, idx, val) in ((cell_rec if in_cols else gene_rec, by_row), (gene_rec if in_cols else cell_rec, by_col)):
                n, i, v = flat(records)
                assert np.array_equal(n, np.diff(ptr)) and np.array_equal(i, idx), s
                assert v.dtype == val.dtype and v.tobytes() == val.tobytes(), s
            pos = data.index(b"\n") + 1
            p = cref.parse(data[pos:], kw.get("sep", ",").encode(), len(cols), "rownames" not in kw, kind, kw.get("null_thresh"), 1)
            if s == "B":
                bad = [f for line in data[pos:].split(b"\n") for f in line.split(b"\t") if f and cref.convert(f, False, 0)[0] != cref.VALUE]
                assert p["stats"]["deferred"] == 0 and not bad, bad
            zeros = 1.0 - p["stats"]["entries"] / p["stats"]["fields"]
            out[s + "_csv"] = np.frombuffer(data, dtype=np.uint8)
            out[s + "_genes"], out[s + "_cells"] = np.array(genes), np.array(cells)
            out[s + "_cell_len"], out[s + "_cell_idx"], out[s + "_cell_val"] = flat(cell_rec)
            out[s + "_gene_len"], out[s + "_gene_idx"], out[s + "_gene_val"] = flat(gene_rec)
            if "inv_log" in kw:
                # numpy's power is not correctly rounded and differs by an ulp between its builds: the values in front of it,
                # which are the parser's alone, are recorded too, from a second run of the reference without inv_log
                raw_fn = os.path.join(tmp, s + "_raw.h5")
                with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
                    ref.csv_to_h5(csv_fn, raw_fn, **{k: v for k, v in ref_kw.items() if k != "inv_log"})
                with h5py.File(raw_fn, "r") as h5:
                    raw_cell, raw_gene = flat([h5["cell_data"][c][:] for c in cells]), flat([h5["gene_data"][g][:] for g in genes])
                assert np.array_equal(raw_cell[1], out[s + "_cell_idx"]) and np.array_equal(raw_gene[1], out[s + "_gene_idx"])
                plain = cref.read_table(data, kw.get("sep", ","), in_cols, None, kind, kw.get("null_thresh"), kw.get("rownames"))
                assert (raw_cell if in_cols else raw_gene)[2].tobytes() == plain[0][2].tobytes() and (raw_gene if in_cols else raw_cell)[2].tobytes() == plain[1][2].tobytes()
                out[s + "_cell_raw"], out[s + "_gene_raw"] = raw_cell[2], raw_gene[2]
            meta[s] = dict(kwargs=kw, dtype=dtypes[0], stats=p["stats"], numpy=np.__version__)
            print("sample %s: %d bytes, %d fields, %d entries (%.0f %% zeros), %d deferred, records %s" % (
                s, len(data), p["stats"]["fields"], p["stats"]["entries"], 100 * zeros, p["stats"]["deferred"], dtypes[0]))
    out["meta"] = np.array(json.dumps(meta))
    fn = os.path.join(GOLD, "csv.npz")
    np.savez_compressed(fn, **out)
    print("wrote %s, %d bytes" % (fn, os.path.getsize(fn)))


if __name__ == "__main__":
    main()
