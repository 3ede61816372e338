"""File-level ingestion (nabo_amd.mtx_to_h5) on the two directories of tests/golden/ingest.npz against what the
reference's mtx_to_h5 wrote from them -- names, dtypes and records, dataset for dataset -- the one stated departure (a
cell without entries gets an EMPTY dataset), the reference's ValueError texts, and on to filter_data on the file
produced.  Needs h5py and a GPU: run by test_ingest_gpu.py under an interpreter with h5py."""
import contextlib
import io
import json
import os
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import nabo_amd  # noqa: E402

nabo_amd._lib.lib()


def main():
    import h5py
    d = np.load(os.path.join(HERE, "golden", "ingest.npz"))
    td = tempfile.mkdtemp()
    differ, checked = [], 0

    def check(what, ok):
        nonlocal checked
        checked += 1
        if not ok:
            differ.append(what)

    try:
        for s in ("A", "B"):
            where = os.path.join(td, s)
            os.makedirs(where)
            pre = s + "_file_"
            for k in d.files:
                if k.startswith(pre):
                    with open(os.path.join(where, k[len(pre):]), "wb") as f:
                        f.write(d[k].tobytes())
            fn = os.path.join(td, s + ".h5")
            with open(fn, "wb") as f:
                f.write(b"not a dataset: to be overwritten")
            with contextlib.redirect_stdout(io.StringIO()) as said:
                nabo_amd.mtx_to_h5(where, fn, batch_size=7)
            check(s + " overwrite notice", said.getvalue() == "Overwriting %s\n" % fn)
            genes, cells = [str(x) for x in d[s + "_genes"]], [str(x) for x in d[s + "_cells"]]
            has = d[s + "_cell_has_dataset"]
            cell_at = np.concatenate([[0], np.cumsum(d[s + "_cell_len"])])
            gene_at = np.concatenate([[0], np.cumsum(d[s + "_gene_len"])])
            rec = np.dtype([("idx", np.uint), ("val", np.int64)])
            with h5py.File(fn, "r") as h5:
                check(s + " groups", sorted(h5.keys()) == ["cell_data", "gene_data", "names"])
                check(s + " gene names", [x.decode() for x in h5["names"]["genes"][:]] == genes)
                check(s + " cell names", [x.decode() for x in h5["names"]["cells"][:]] == cells)
                check(s + " every cell and gene has a dataset", sorted(h5["cell_data"].keys()) == sorted(cells) and sorted(h5["gene_data"].keys()) == sorted(genes))
                ok_dtype = ok_cells = ok_genes = ok_empty = True
                k = 0
                for c, name in enumerate(cells):
                    r = h5["cell_data"][name][:]
                    ok_dtype &= r.dtype == rec
                    if has[c]:
                        ok_cells &= np.array_equal(r["idx"], d[s + "_cell_idx"][cell_at[k]:cell_at[k + 1]]) and np.array_equal(r["val"], d[s + "_cell_val"][cell_at[k]:cell_at[k + 1]])
                        k += 1
                    else:
                        ok_empty &= r.shape == (0,)
                for g, name in enumerate(genes):
                    r = h5["gene_data"][name][:]
                    ok_dtype &= r.dtype == rec
                    ok_genes &= np.array_equal(r["idx"], d[s + "_gene_idx"][gene_at[g]:gene_at[g + 1]]) and np.array_equal(r["val"], d[s + "_gene_val"][gene_at[g]:gene_at[g + 1]])
                check(s + " dtypes", bool(ok_dtype))
                check(s + " cell records", bool(ok_cells) and k == int(has.sum()))
                check(s + " gene records", bool(ok_genes))
                check(s + " cells without entries have empty datasets", bool(ok_empty) and int((~has).sum()) == 2)
            # another value type
            fn32 = os.path.join(td, s + "_u32.h5")
            nabo_amd.mtx_to_h5(where, fn32, value_dtype=np.uint32)
            with h5py.File(fn32, "r") as h5:
                r = h5["cell_data"][cells[1]][:]
                check(s + " value_dtype", r.dtype == np.dtype([("idx", np.uint), ("val", np.uint32)]) and int(r["val"][0]) == 2 ** 31 + 12345)
            # the file is a dataset the next step reads
            with contextlib.redirect_stdout(io.StringIO()):
                kc, kg = nabo_amd.filter_data(fn, min_exp=10, min_ngenes=5, min_gene_abundance=1)
            check(s + " filter_data", 250 < len(kc) <= 297 and 150 < len(kg) <= 197)
        # the count checks, with the reference's texts
        for drop, text in (("genes.tsv", "Number of gene in genes.tsv not same as in the mtx file"),
                           ("barcodes.tsv", "Number of cells in barcodes.tsv not same as in the mtx file")):
            where = os.path.join(td, "short_" + drop)
            shutil.copytree(os.path.join(td, "A"), where)
            lines = open(os.path.join(where, drop), "rb").read().splitlines(True)
            with open(os.path.join(where, drop), "wb") as f:
                f.write(b"".join(lines[:-1]))
            try:
                nabo_amd.mtx_to_h5(where, os.path.join(td, "short.h5"))
                check("refusal of a short " + drop, False)
            except ValueError as e:
                check("refusal of a short " + drop, str(e) == text)
    finally:
        shutil.rmtree(td, ignore_errors=True)
    print("RESULT " + json.dumps({"checked": checked, "differ": differ}))


if __name__ == "__main__":
    main()
