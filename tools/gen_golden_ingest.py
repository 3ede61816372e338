#!/opt/conda/bin/python3.9
"""Golden vectors for the Matrix Market reader: what the reference's mtx_to_h5 (nabo/_io.py:61-235) writes.

TEST INFRASTRUCTURE ONLY, run where the reference is mounted, with an interpreter that has h5py, numpy and tqdm:

    /opt/conda/bin/python3.9 tools/gen_golden_ingest.py

The reference's nabo/_io.py is loaded BY FILE PATH (it imports nothing of its package).  Two seeded directories of 300
cells x 200 genes with about 6 000 entries are written into a temporary directory, the reference's own mtx_to_h5 runs
on them, and only DATA goes to tests/golden/ingest.npz: the BYTES of the input files and, from the file the reference
wrote, the names, the concatenated cell_data and gene_data records, their lengths, and which cells got a dataset.

Directory A: plain files in 10x order (by cell, genes ascending inside a cell) with gene names that collide only after
upper-casing, lower-case barcodes, empty cells including the first and the last, empty genes, header comment lines and
one value above 2^31.  Directory B: the same pattern from another seed as .gz files, with a three-column features.tsv.gz.

Asserted, so that the tests can demand equality: the plain restatement (tests/_ingest_ref.py: the grammar, two stable
sorts, fix_dup_names) reproduces every record and every name the reference wrote; the reference wrote a dataset for
every cell with entries.
"""
import contextlib
import gzip
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
import _ingest_ref as iref  # noqa: E402

N_CELLS, N_GENES = 300, 200
MAX_LINE = 1024                     # (no line of these files comes near it)
EMPTY_CELLS = (0, 137, N_CELLS - 1)
EMPTY_GENES = (4, 150, N_GENES - 1)
BIG_VALUE = 2 ** 31 + 12345
SAMPLES = {"A": dict(seed=20241101, gz=False), "B": dict(seed=20241102, gz=True)}


def load_reference():
    spec = importlib.util.spec_from_file_location("nabo_ref_io", os.path.join(REF, "nabo", "_io.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def make_files(seed, gz):
    """{file name: bytes} of one directory"""
    rng = np.random.default_rng(seed)
    lines, first = [], True
    for c in range(N_CELLS):
        if c in EMPTY_CELLS:
            continue
        genes = np.sort(rng.choice([g for g in range(N_GENES) if g not in EMPTY_GENES], size=int(rng.integers(8, 34)), replace=False))
        for g in genes.tolist():
            v = BIG_VALUE if first else int(rng.integers(1, 60))
            first = False
            lines.append("%d %d %d" % (g + 1, c + 1, v))
    head = "%%MatrixMarket matrix coordinate integer general\n%metadata_json: {\"format_version\": 2}\n%\n"
    mtx = (head + "%d %d %d\n" % (N_GENES, N_CELLS, len(lines)) + "\n".join(lines) + "\n").encode()
    names = ["Gene%d" % g for g in range(N_GENES)]
    names[10], names[11], names[12] = "Abc1", "ABC1", "abc1"        # collide only in upper case
    names[60], names[61] = "Xy", "xY"
    if gz:
        genes_tsv = "".join("ENSG%05d\t%s\tGene Expression\n" % (g, n) for g, n in enumerate(names)).encode()
    else:
        genes_tsv = "".join("ENSG%05d\t%s\n" % (g, n) for g, n in enumerate(names)).encode()
    codes = ["".join("acgt"[int(x)] for x in rng.integers(0, 4, size=14)) + "-%d" % (c % 3 + 1) for c in range(N_CELLS)]
    assert len(set(codes)) == N_CELLS
    barcodes = "".join(c + "\n" for c in codes).encode()
    if gz:
        pack = lambda b: gzip.compress(b, mtime=0)  # noqa: E731
        return {"matrix.mtx.gz": pack(mtx), "features.tsv.gz": pack(genes_tsv), "barcodes.tsv.gz": pack(barcodes)}
    return {"matrix.mtx": mtx, "genes.tsv": genes_tsv, "barcodes.tsv": barcodes}


def plain(files, stem):
    for name, data in files.items():
        if name.startswith(stem):
            return gzip.decompress(data) if name.endswith(".gz") else data
    raise KeyError(stem)


def main():
    ref = load_reference()
    out, meta = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        for s, cfg in SAMPLES.items():
            d = os.path.join(tmp, s)
            os.makedirs(d)
            files = make_files(cfg["seed"], cfg["gz"])
            for name, data in files.items():
                with open(os.path.join(d, name), "wb") as f:
                    f.write(data)
            h5_fn = os.path.join(tmp, s + ".h5")
            with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
                ref.mtx_to_h5(d, h5_fn)
            with h5py.File(h5_fn, "r") as h5:
                genes = [x.decode() for x in h5["names"]["genes"][:]]
                cells = [x.decode() for x in h5["names"]["cells"][:]]
                has = np.array([c in h5["cell_data"] for c in cells])
                cell_rec = [h5["cell_data"][c][:] for c in cells if c in h5["cell_data"]]
                gene_rec = [h5["gene_data"][g][:] for g in genes]
                assert all(r.dtype == np.dtype([("idx", np.uint), ("val", np.int64)]) for r in cell_rec + gene_rec)
            # the restatement reproduces all of it
            parsed = iref.parse(plain(files, "matrix.mtx"), MAX_LINE)
            (cell_ptr, gene, val), (gene_ptr, cell, gval) = iref.csr_csc(parsed)
            assert genes == iref.fix_dup_names(iref.second_column(plain(files, "genes.tsv" if not cfg["gz"] else "features.tsv")))
            assert cells == iref.barcodes(plain(files, "barcodes.tsv"))
            n_ent = np.diff(cell_ptr)
            assert (has[n_ent > 0]).all(), "the reference left out a cell with entries"
            k = 0
            for c in range(N_CELLS):
                if has[c]:
                    r = cell_rec[k]
                    k += 1
                    assert np.array_equal(r["idx"], gene[cell_ptr[c]:cell_ptr[c + 1]]) and np.array_equal(r["val"], val[cell_ptr[c]:cell_ptr[c + 1]]), c
            for g in range(N_GENES):
                r = gene_rec[g]
                assert np.array_equal(r["idx"], cell[gene_ptr[g]:gene_ptr[g + 1]]) and np.array_equal(r["val"], gval[gene_ptr[g]:gene_ptr[g + 1]]), g
            assert int(val.max()) == BIG_VALUE and all(n_ent[c] == 0 for c in EMPTY_CELLS) and all(np.diff(gene_ptr)[g] == 0 for g in EMPTY_GENES)
            for name, data in files.items():
                out["%s_file_%s" % (s, name)] = np.frombuffer(data, dtype=np.uint8)
            out[s + "_genes"], out[s + "_cells"] = np.array(genes), np.array(cells)
            out[s + "_cell_has_dataset"] = has
            out[s + "_cell_len"] = np.array([len(r) for r in cell_rec], dtype=np.int64)
            out[s + "_cell_idx"] = np.concatenate([r["idx"] for r in cell_rec]).astype(np.int64)
            out[s + "_cell_val"] = np.concatenate([r["val"] for r in cell_rec]).astype(np.int64)
            out[s + "_gene_len"] = np.array([len(r) for r in gene_rec], dtype=np.int64)
            out[s + "_gene_idx"] = np.concatenate([r["idx"] for r in gene_rec]).astype(np.int64)
            out[s + "_gene_val"] = np.concatenate([r["val"] for r in gene_rec]).astype(np.int64)
            meta[s] = dict(files=sorted(files), nnz=int(len(val)), empty_cells=list(EMPTY_CELLS), empty_genes=list(EMPTY_GENES),
                           cells_without_dataset=[int(c) for c in np.flatnonzero(~has)], big_value=BIG_VALUE)
            print("sample %s: %d entries, %d of %d cells have a dataset (empty cells %s)" % (s, len(val), int(has.sum()), N_CELLS, list(EMPTY_CELLS)))
    out["meta"] = np.array(json.dumps(meta))
    fn = os.path.join(GOLD, "ingest.npz")
    np.savez_compressed(fn, **out)
    print("wrote %s, %d bytes" % (fn, os.path.getsize(fn)))


if __name__ == "__main__":
    main()
