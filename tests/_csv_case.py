"""File-level ingestion (nabo_amd.csv_to_h5) on sample A of tests/golden/csv.npz against what the reference's csv_to_h5
wrote from it -- names, dtypes and records, dataset for dataset -- and the overwrite notice.  Needs h5py and a GPU: run by
test_csv_gpu.py under an interpreter with h5py."""
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
    d = np.load(os.path.join(HERE, "golden", "csv.npz"))
    meta = json.loads(str(d["meta"]))["A"]
    td = tempfile.mkdtemp()
    differ, checked = [], 0

    def check(what, ok):
        nonlocal checked
        checked += 1
        if not ok:
            differ.append(what)

    try:
        csv_fn, fn = os.path.join(td, "A.csv"), os.path.join(td, "A.h5")
        with open(csv_fn, "wb") as f:
            f.write(d["A_csv"].tobytes())
        with open(fn, "wb") as f:
            f.write(b"not a dataset: to be overwritten")
        with contextlib.redirect_stdout(io.StringIO()) as said:
            nabo_amd.csv_to_h5(csv_fn, fn, batch_size=7, **meta["kwargs"])
        check("overwrite notice", said.getvalue() == "Overwriting %s\n" % fn)
        genes, cells = [str(x) for x in d["A_genes"]], [str(x) for x in d["A_cells"]]
        rec = np.dtype([("idx", np.int64), ("val", np.float64)])
        check("the reference's dtype", str(rec) == meta["dtype"])
        with h5py.File(fn, "r") as h5:
            check("groups", sorted(h5.keys()) == ["cell_data", "gene_data", "names"])
            check("gene names", [x.decode() for x in h5["names"]["genes"][:]] == genes)
            check("cell names", [x.decode() for x in h5["names"]["cells"][:]] == cells)
            check("every cell and gene has a dataset", sorted(h5["cell_data"].keys()) == sorted(cells) and sorted(h5["gene_data"].keys()) == sorted(genes))
            for group, names in (("cell", cells), ("gene", genes)):
                at = np.concatenate([[0], np.cumsum(d["A_%s_len" % group])])
                ok_dtype = ok_rec = True
                for k, name in enumerate(names):
                    r = h5[group + "_data"][name][:]
                    ok_dtype &= r.dtype == rec
                    ok_rec &= r["idx"].tobytes() == d["A_%s_idx" % group][at[k]:at[k + 1]].tobytes() and r["val"].tobytes() == d["A_%s_val" % group][at[k]:at[k + 1]].tobytes()
                check(group + " dtypes", bool(ok_dtype))
                check(group + " records", bool(ok_rec))
    finally:
        shutil.rmtree(td, ignore_errors=True)
    print("RESULT " + json.dumps({"checked": checked, "differ": differ}))


if __name__ == "__main__":
    main()
