#!/opt/conda/bin/python3.9
"""Golden vectors for the Matrix Market writer and for subsetting and merging counts: what the reference's h5_to_mtx
(nabo/_io.py:645-674), extract_cells_from_h5 (:597-642) and merge_h5 (:502-594) write.

TEST INFRASTRUCTURE ONLY, run where the reference is mounted, with an interpreter that has h5py, numpy, pandas and tqdm:

    /opt/conda/bin/python3.9 tools/gen_golden_counts.py

The reference's nabo/_io.py and nabo/_dataset.py are loaded BY FILE PATH under a fake `nabo` package (as
tools/gen_golden_qc.py does), so that h5_to_mtx's `from ._dataset import Dataset` resolves.  The two dataset files are
built with h5py from the restated indexes (tests/_ingest_ref.py) of the golden directories A and B of
tests/golden/ingest.npz, with a dataset for EVERY cell, the empty ones included: the reference's own h5_to_mtx fails on a
cell without one.  Then, in a temporary working directory (h5_to_mtx writes nabo.temp1 / nabo.temp2 there):
h5_to_mtx of A and of B; extract_cells_from_h5 of A with a seeded third of its cells (and two names that are not in
the file); merge_h5 of A + B after random.seed(MERGE_SEED).  Only DATA goes to tests/golden/counts.npz: the bytes of the
written files, the names, and the records of the extracted and of the merged file.  A function of the reference that
fails is recorded as failing in `meta`, with its exception, and not worked around.

Asserted, so that the tests can demand equality: the plain restatement (tests/_counts_ref.py) reproduces every byte and
every record; records are compared after sorting by index where the reference leaves them unsorted (the gene records of
the merged file are in concatenation order).
"""
import contextlib
import importlib.util
import io
import json
import os
import random
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
REF = os.environ.get("NABO_REFERENCE", "/root/reference")
GOLD = os.path.join(REPO, "tests", "golden")
sys.path.insert(0, os.path.join(REPO, "tests"))
import _counts_ref as cref  # noqa: E402
import _ingest_ref as iref  # noqa: E402

MAX_LINE = 1024
EXTRACT_SEED, MERGE_SEED = 20241201, 20241202
COMMENT = b'%metadata_json: {"format_version": 2, "software_version": "3.0.2"}\n'


def load_reference():
    nb = types.ModuleType("numba")
    nb.jit = lambda *a, **k: (a[0] if len(a) == 1 and callable(a[0]) and not k else (lambda f: f))
    sys.modules["numba"] = nb
    pkg = types.ModuleType("nabo")
    pkg.__path__ = []
    sys.modules["nabo"] = pkg
    plot = types.ModuleType("nabo._plotting")
    plot.plot_mean_var = lambda *a, **k: None
    plot.plot_summary_data = lambda *a, **k: None
    sys.modules["nabo._plotting"] = plot
    mods = {}
    for name in ("_dataset", "_io"):
        spec = importlib.util.spec_from_file_location("nabo." + name, os.path.join(REF, "nabo", name + ".py"))
        mods[name] = importlib.util.module_from_spec(spec)
        sys.modules["nabo." + name] = mods[name]
        spec.loader.exec_module(mods[name])
    return mods["_io"]


def quiet(fn, *a, **k):
    """(result, None) or (None, 'ExceptionType: text'); what the call printed is dropped"""
    with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
        try:
            return fn(*a, **k), None
        except Exception as e:  # recorded, not worked around
            return None, "%s: %s" % (type(e).__name__, e)


def mtx_of(d, s):
    import gzip
    pre = s + "_file_"
    f = {k[len(pre):]: d[k].tobytes() for k in d.files if k.startswith(pre)}
    return f["matrix.mtx"] if "matrix.mtx" in f else gzip.decompress(f["matrix.mtx.gz"])


def names_of(fn):
    import h5py
    with h5py.File(fn, "r") as h5:
        return [x.decode() for x in h5["names"]["genes"][:]], [x.decode() for x in h5["names"]["cells"][:]]


def same(a, b):
    return all(np.array_equal(np.asarray(x).astype(np.int64), np.asarray(y).astype(np.int64)) for x, y in zip(a, b))


def flat(index):
    """(lengths, idx, val) of a (ptr, idx, val)"""
    return np.diff(index[0]), index[1], index[2]


def main():
    ref = load_reference()
    ingest = np.load(os.path.join(GOLD, "ingest.npz"))
    out, meta, data = {}, {}, {}
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            for s in ("A", "B"):
                parsed = iref.parse(mtx_of(ingest, s), MAX_LINE)
                csr, csc = iref.csr_csc(parsed)
                genes, cells = [str(x) for x in ingest[s + "_genes"]], [str(x) for x in ingest[s + "_cells"]]
                fn = os.path.join(tmp, s + ".h5")
                cref.write_dataset(fn, genes, cells, csr, csc)
                data[s] = dict(fn=fn, genes=genes, cells=cells, csr=csr, csc=csc, n_genes=parsed[0])
                # ---- h5_to_mtx
                outdir = os.path.join(tmp, s + "_mtx")
                os.makedirs(outdir)
                _, err = quiet(ref.h5_to_mtx, fn, outdir)
                meta["h5_to_mtx_" + s] = err
                if err is None:
                    files = {n: open(os.path.join(outdir, n), "rb").read() for n in ("matrix.mtx", "genes.tsv", "barcodes.tsv")}
                    assert files["matrix.mtx"] == cref.mtx_text(parsed[0], csr[0], csr[1], csr[2], COMMENT, blank=True), "h5_to_mtx text of " + s
                    assert files["genes.tsv"] == "".join(g + "\t" + g + "\n" for g in genes).encode()
                    assert files["barcodes.tsv"] == "".join(c + "\n" for c in cells).encode()
                    assert not os.path.exists("nabo.temp1") and not os.path.exists("nabo.temp2")
                    for n, b in files.items():
                        out["%s_mtx_file_%s" % (s, n)] = np.frombuffer(b, dtype=np.uint8)
                print("h5_to_mtx %s: %s" % (s, err or "%d bytes of matrix.mtx" % len(files["matrix.mtx"])))
            # ---- extract_cells_from_h5: a seeded third of A's cells, in shuffled order, and two strangers
            a = data["A"]
            rng = np.random.default_rng(EXTRACT_SEED)
            coi = [a["cells"][i] for i in rng.permutation(len(a["cells"]))[:len(a["cells"]) // 3]] + ["NOT-A-CELL-1", "NOT-A-CELL-2"]
            ex_fn = os.path.join(tmp, "extract.h5")
            _, err = quiet(ref.extract_cells_from_h5, a["fn"], ex_fn, coi)
            meta["extract"] = err
            out["extract_coi"] = np.array(coi)
            if err is None:
                genes, cells = names_of(ex_fn)
                rows = [n for n, c in enumerate(a["cells"]) if c in set(coi)]
                assert genes == a["genes"] and cells == [a["cells"][r] for r in rows], "extract keeps file order and all genes"
                cell_rec, gene_rec = cref.read_records(ex_fn, "cell_data", cells), cref.read_records(ex_fn, "gene_data", genes)
                want = cref.subset(a["csr"][0], a["csr"][1], a["csr"][2], a["n_genes"], rows)
                assert same(cell_rec, flat(want[0])) and same(gene_rec, flat(want[1])), "extract records"
                out["extract_genes"], out["extract_cells"] = np.array(genes), np.array(cells)
                for k, r in (("cell", cell_rec), ("gene", gene_rec)):
                    out["extract_%s_len" % k], out["extract_%s_idx" % k], out["extract_%s_val" % k] = r
            print("extract_cells_from_h5: %s" % (err or "%d of %d cells" % (len(cells), len(coi))))
            # ---- merge_h5 of A + B
            b = data["B"]
            mg_fn = os.path.join(tmp, "merged.h5")
            random.seed(MERGE_SEED)
            _, err = quiet(ref.merge_h5, [a["fn"], b["fn"]], mg_fn, ["s1", "s2"])
            meta["merge"] = err
            if err is None:
                genes, cells = names_of(mg_fn)
                cell_rec, gene_rec = cref.read_records(mg_fn, "cell_data", cells), cref.read_records(mg_fn, "gene_data", genes)
                want = cref.merge([a["csr"], b["csr"]], [a["genes"], b["genes"]], [a["cells"], b["cells"]], ["s1", "s2"], cells)
                assert genes == want[2] and sorted(cells) == sorted([c + "-s1" for c in a["cells"]] + [c + "-s2" for c in b["cells"]])
                unsorted_genes = not same(gene_rec, cref.sorted_records(*gene_rec))
                assert same(cref.sorted_records(*cell_rec), flat(want[0])) and same(cref.sorted_records(*gene_rec), flat(want[1])), "merge records"
                meta["merge_gene_records_unsorted"] = bool(unsorted_genes)
                out["merge_genes"], out["merge_cells"] = np.array(genes), np.array(cells)
                for k, r in (("cell", cell_rec), ("gene", gene_rec)):
                    out["merge_%s_len" % k], out["merge_%s_idx" % k], out["merge_%s_val" % k] = r
            print("merge_h5: %s" % (err or "%d genes, %d cells, gene records unsorted: %s" % (len(genes), len(cells), unsorted_genes)))
        finally:
            os.chdir(cwd)
    out["meta"] = np.array(json.dumps(meta))
    fn = os.path.join(GOLD, "counts.npz")
    np.savez_compressed(fn, **out)
    print("wrote %s, %d bytes" % (fn, os.path.getsize(fn)))


if __name__ == "__main__":
    main()
