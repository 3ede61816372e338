"""The file-level functions on counts (nabo_amd.extract_cells_from_h5, merge_h5, h5_to_mtx, read_h5_counts) against what
the reference wrote from the same two dataset files (tests/golden/counts.npz, tools/gen_golden_counts.py): the files are
rebuilt with h5py from the restated indexes of the golden directories A and B, as the tool built them.  Records are
compared after sorting by index where the reference leaves them unsorted (the gene records of its merged file).  Also:
the reference's errors and its warning, files with different gene sets (where the reference fails), the round trip
h5_to_mtx -> mtx_to_h5, and the stated departures.  Needs h5py and a GPU: run by test_counts_gpu.py under an interpreter
with h5py."""
import contextlib
import hashlib
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
import _counts_ref as cref  # noqa: E402
import _ingest_ref as iref  # noqa: E402

nabo_amd._lib.lib()


def golden_matrix(d, s):
    import gzip
    pre = s + "_file_"
    f = {k[len(pre):]: d[k].tobytes() for k in d.files if k.startswith(pre)}
    parsed = iref.parse(f["matrix.mtx"] if "matrix.mtx" in f else gzip.decompress(f["matrix.mtx.gz"]), 1024)
    csr, csc = iref.csr_csc(parsed)
    return dict(n_genes=parsed[0], csr=csr, csc=csc, genes=[str(x) for x in d[s + "_genes"]], cells=[str(x) for x in d[s + "_cells"]])


def names_of(fn):
    import h5py
    with h5py.File(fn, "r") as h5:
        return [x.decode() for x in h5["names"]["genes"][:]], [x.decode() for x in h5["names"]["cells"][:]], sorted(h5.keys()), \
            len(h5["cell_data"]), len(h5["gene_data"]), h5["cell_data"][h5["names"]["cells"][0].decode()].dtype


def same(a, b):
    return all(np.array_equal(np.asarray(x).astype(np.int64), np.asarray(y).astype(np.int64)) for x, y in zip(a, b))


def flat(index):
    return np.diff(index[0]), index[1], index[2]


def digest(fn):
    with open(fn, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def main():
    import h5py
    ingest, gold = np.load(os.path.join(HERE, "golden", "ingest.npz")), np.load(os.path.join(HERE, "golden", "counts.npz"))
    td = tempfile.mkdtemp()
    differ, checked = [], 0
    rec = np.dtype([("idx", np.uint), ("val", np.int64)])

    def check(what, ok):
        nonlocal checked
        checked += 1
        if not ok:
            differ.append(what)

    def raises(kind, text, fn, *a, **k):
        try:
            with contextlib.redirect_stdout(io.StringIO()):
                fn(*a, **k)
        except kind as e:
            return text is None or text in str(e)
        except Exception:
            return False
        return False

    try:
        data = {}
        for s in ("A", "B"):
            data[s] = golden_matrix(ingest, s)
            data[s]["fn"] = os.path.join(td, s + ".h5")
            cref.write_dataset(data[s]["fn"], data[s]["genes"], data[s]["cells"], data[s]["csr"], data[s]["csc"])
        a, b = data["A"], data["B"]
        before = {s: digest(data[s]["fn"]) for s in data}

        # ---- read_h5_counts
        m, genes, cells = nabo_amd.read_h5_counts(a["fn"])
        check("read_h5_counts", genes == a["genes"] and cells == a["cells"] and same((m.cell_ptr, m.gene, m.val), a["csr"])
              and same((m.gene_ptr, m.cell, m.gene_val), a["csc"]) and m.val.dtype == np.uint32)

        # ---- extract_cells_from_h5
        coi = [str(x) for x in gold["extract_coi"]]
        ex = os.path.join(td, "extract.h5")
        with open(ex, "wb") as f:
            f.write(b"to be overwritten")
        with contextlib.redirect_stdout(io.StringIO()) as said:
            nabo_amd.extract_cells_from_h5(a["fn"], ex, coi)
        check("extract warning", said.getvalue() == "WARNING: only 100/102 cells found in the H5 file\n")
        genes, cells, groups, n_cd, n_gd, dt = names_of(ex)
        check("extract names", genes == [str(x) for x in gold["extract_genes"]] and cells == [str(x) for x in gold["extract_cells"]])
        check("extract groups and dtype", groups == ["cell_data", "gene_data", "names"] and (n_cd, n_gd) == (100, 200) and dt == rec)
        check("extract cell records", same(cref.read_records(ex, "cell_data", cells), [gold["extract_cell_" + k] for k in ("len", "idx", "val")]))
        check("extract gene records", same(cref.read_records(ex, "gene_data", genes), [gold["extract_gene_" + k] for k in ("len", "idx", "val")]))
        check("extract of no known cell", raises(ValueError, "ERROR: None of the input cells were found in the H5 file", nabo_amd.extract_cells_from_h5,
                                                 a["fn"], os.path.join(td, "none.h5"), ["NOBODY"]))
        with contextlib.redirect_stdout(io.StringIO()) as said:
            nabo_amd.extract_cells_from_h5(a["fn"], ex, cells[:5])
        check("extract without warning", said.getvalue() == "" and names_of(ex)[1] == cells[:5])

        # ---- merge_h5, the golden's cell order given
        mg = os.path.join(td, "merged.h5")
        order = [str(x) for x in gold["merge_cells"]]
        with contextlib.redirect_stdout(io.StringIO()):
            nabo_amd.merge_h5([a["fn"], b["fn"]], mg, ["s1", "s2"], cell_order=order)
        genes, cells, groups, n_cd, n_gd, dt = names_of(mg)
        check("merge names", genes == [str(x) for x in gold["merge_genes"]] and cells == order)
        check("merge groups and dtype", groups == ["cell_data", "gene_data", "names"] and (n_cd, n_gd) == (600, 200) and dt == rec)
        want_cell = cref.sorted_records(*[gold["merge_cell_" + k] for k in ("len", "idx", "val")])
        want_gene = cref.sorted_records(*[gold["merge_gene_" + k] for k in ("len", "idx", "val")])
        check("merge cell records", same(cref.read_records(mg, "cell_data", cells), want_cell))
        check("merge gene records", same(cref.read_records(mg, "gene_data", genes), want_gene))
        # the default: suffixes 1, 2, ... and a permutation the seed decides
        with contextlib.redirect_stdout(io.StringIO()):
            nabo_amd.merge_h5([a["fn"], b["fn"]], mg)
            first = names_of(mg)[1]
            nabo_amd.merge_h5([a["fn"], b["fn"]], mg)
            again = names_of(mg)[1]
            nabo_amd.merge_h5([a["fn"], b["fn"]], mg, seed=1)
            other = names_of(mg)[1]
        concat = [c + "-1" for c in a["cells"]] + [c + "-2" for c in b["cells"]]
        check("merge default order", first == again and first != other and first != concat and sorted(first) == sorted(concat) == sorted(other))
        check("merge refuses a wrong number of suffixes", raises(ValueError, "ERROR: Number of cell_suffixes not same as number of input H5 files",
                                                                 nabo_amd.merge_h5, [a["fn"], b["fn"]], mg, ["x"]))
        lacking = os.path.join(td, "lacking.h5")
        shutil.copy(a["fn"], lacking)
        with h5py.File(lacking, "a") as h5:
            del h5["gene_data"]
        check("merge refuses a file without gene_data", raises(KeyError, "ERROR: Group gene_data missing in file %s" % lacking, nabo_amd.merge_h5,
                                                               [a["fn"], lacking], mg))

        # ---- different gene sets: the true union (the reference raises KeyError here)
        c_genes = ["NEW%d" % i if i % 9 == 2 else g for i, g in enumerate(b["genes"])][::-1]
        n_g = b["n_genes"]
        back = cref.remap(*b["csr"], list(range(300)), list(range(n_g - 1, -1, -1)), n_g)            # B with its genes in reverse order
        rev = os.path.join(td, "C.h5")
        cref.write_dataset(rev, c_genes, b["cells"], back[0], back[1])
        with contextlib.redirect_stdout(io.StringIO()):
            nabo_amd.merge_h5([a["fn"], rev], mg, ["p", "q"], cell_order=[c + "-q" for c in b["cells"]] + [c + "-p" for c in a["cells"]][::-1])
        genes, cells = names_of(mg)[:2]
        want = cref.merge([a["csr"], back[0]], [a["genes"], c_genes], [a["cells"], b["cells"]], ["p", "q"], cells)
        check("union of different gene sets", genes == want[2] == sorted(set(a["genes"]) | set(c_genes)) and len(genes) > 200)
        check("union cell records", same(cref.read_records(mg, "cell_data", cells), flat(want[0])))
        check("union gene records", same(cref.read_records(mg, "gene_data", genes), flat(want[1])))

        # ---- h5_to_mtx: the reference's bytes; and back through mtx_to_h5
        for s in ("A", "B"):
            outdir = os.path.join(td, s + "_mtx")
            os.makedirs(outdir)
            nabo_amd.h5_to_mtx(data[s]["fn"], outdir)
            ok = sorted(os.listdir(outdir)) == ["barcodes.tsv", "genes.tsv", "matrix.mtx"]
            for n in ("matrix.mtx", "genes.tsv", "barcodes.tsv"):
                ok = ok and open(os.path.join(outdir, n), "rb").read() == gold["%s_mtx_file_%s" % (s, n)].tobytes()
            check(s + " h5_to_mtx files", ok)
            round_fn = os.path.join(td, s + "_round.h5")
            with contextlib.redirect_stdout(io.StringIO()):
                nabo_amd.mtx_to_h5(outdir, round_fn)
            d = data[s]
            check(s + " round trip names", names_of(round_fn)[:2] == (d["genes"], d["cells"]) and names_of(round_fn)[2:] == names_of(d["fn"])[2:])
            check(s + " round trip records", same(cref.read_records(round_fn, "cell_data", d["cells"]), cref.read_records(d["fn"], "cell_data", d["cells"]))
                  and same(cref.read_records(round_fn, "gene_data", d["genes"]), cref.read_records(d["fn"], "gene_data", d["genes"])))
        check("the input files are untouched", all(digest(data[s]["fn"]) == before[s] for s in data))
        # values that are not integers are refused; a cell without a dataset has no entries
        real = os.path.join(td, "real.h5")
        vals = a["csr"][2].astype(np.float64)
        vals[7] = 2.5
        cref.write_dataset(real, a["genes"], a["cells"], (a["csr"][0], a["csr"][1], vals), a["csc"], value_dtype=np.float64)
        outdir = os.path.join(td, "real_mtx")
        os.makedirs(outdir)
        check("h5_to_mtx refuses real values", raises(ValueError, "must be integers", nabo_amd.h5_to_mtx, real, outdir) and os.listdir(outdir) == [])
        with h5py.File(lacking, "a") as h5:
            del h5["cell_data"][a["cells"][1]]
        m = nabo_amd.read_h5_counts(lacking)[0]
        check("a cell without a dataset", m.cell_ptr[1] == m.cell_ptr[2] and m.nnz == len(a["csr"][1]) - int(np.diff(a["csr"][0])[1]))
    finally:
        shutil.rmtree(td, ignore_errors=True)
    print("RESULT " + json.dumps({"checked": checked, "differ": differ}))


if __name__ == "__main__":
    main()
