"""File-level quality control (nabo_amd.filter_data, set_sf, qc_and_sf, gene_stats, correct_var, find_hvgs, dump_hvgs) on
Nabo-format dataset files written from tests/golden/qc.npz, against what the reference computed from the same files, and
on to fit_pca and transform_pca.  Needs h5py and a GPU: run by test_qc_gpu.py under an interpreter with h5py."""
import contextlib
import io
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import _qc_ref as qref  # noqa: E402

import nabo_amd  # noqa: E402

nabo_amd._lib.lib()          # before pandas comes in: its numexpr may bring an older libstdc++ than the library needs


def write_dataset(fn, d, s, pre):
    """names/{cells,genes}, gene_data/<gene> and cell_data/<cell> as (idx, val) records; processed_data only with `pre`"""
    import h5py
    rec = [("idx", np.uint32), ("val", np.float32)]
    ptr, gene, val = d["cell_ptr"], d["gene"], d[s + "_val"]
    cell = np.repeat(np.arange(ptr.shape[0] - 1), np.diff(ptr))
    o = np.argsort(gene, kind="stable")                          # gene-major, cells ascending inside a gene
    gptr = np.concatenate([[0], np.cumsum(np.bincount(gene, minlength=len(d["genes"])))])
    with h5py.File(fn, "w") as h5:
        g = h5.create_group("names")
        g.create_dataset("cells", data=np.array([str(x).encode() for x in d["cells"]]))
        g.create_dataset("genes", data=np.array([str(x).encode() for x in d["genes"]]))
        for grp, names, p, idx, v in (("gene_data", d["genes"], gptr, cell[o], val[o]), ("cell_data", d["cells"], ptr, gene, val)):
            hg = h5.create_group(grp)
            for j, name in enumerate(names):
                r = np.zeros(int(p[j + 1] - p[j]), dtype=rec)
                r["idx"], r["val"] = idx[p[j]:p[j + 1]], v[p[j]:p[j + 1]]
                hg.create_dataset(str(name), data=r)
        if pre:
            pg = h5.create_group("processed_data")
            pg.create_dataset("keep_cells_idx", data=d["pre_cells"])
            pg.create_dataset("keep_genes_idx", data=d["pre_genes"])


def stored(fn, name):
    import h5py
    with h5py.File(fn, "r") as h5:
        return h5["processed_data"][name][:]


def main():
    d = np.load(os.path.join(HERE, "golden", "qc.npz"))
    td = tempfile.mkdtemp()
    mp, rp = qref.patterns_of(d)
    differ, checked = [], 0

    def check(what, ok):
        nonlocal checked
        checked += 1
        if not ok:
            differ.append(what)

    for s in ("A", "B"):
        thr = qref.thresholds_of(d, s)
        for pre in ("", "_pre"):
            fn = os.path.join(td, s + pre + ".h5")
            write_dataset(fn, d, s, bool(pre))
            with contextlib.redirect_stdout(io.StringIO()) as out:
                kc, kg = nabo_amd.filter_data(fn, mito_patterns=mp, ribo_patterns=rp, **thr)
            tag = s + pre
            check(tag + " report", out.getvalue().splitlines() == [str(x) for x in d[tag + "_report"]])
            for name, got in (("keep_cells", kc), ("keep_genes", kg)):
                w = stored(fn, name + "_idx")
                check(tag + " " + name, w.dtype == np.int64 and np.array_equal(w, d[tag + "_" + name]) and np.array_equal(got, w))
            for name, kw in (("sf_all", {"all_genes": True}), ("sf_scale", {"size_scale": 1234.567}), ("sf", {})):
                sf = nabo_amd.set_sf(fn, **kw)
                w = stored(fn, "sf")
                ref = d[tag + "_" + name]
                same = np.array_equal(w.view(np.int32), ref.view(np.int32)) if s == "A" else np.allclose(w, ref, rtol=4 * float(d["tot_dev"]) + 2.0 ** -23, atol=0)
                check(tag + " " + name, w.dtype == np.float32 and w.shape == ref.shape and same and np.array_equal(sf, w))
            # the one-pass form on a fresh file writes the same three datasets
            fn2 = os.path.join(td, s + pre + "_once.h5")
            write_dataset(fn2, d, s, bool(pre))
            with contextlib.redirect_stdout(io.StringIO()):
                nabo_amd.qc_and_sf(fn2, mito_patterns=mp, ribo_patterns=rp, **thr)
            check(tag + " one pass", all(np.array_equal(stored(fn, k), stored(fn2, k)) for k in ("keep_cells_idx", "keep_genes_idx", "sf")))

    # ---- sample A, no lists beforehand: statistics, correction, HVGs, and on to the PCA
    fn = os.path.join(td, "A.h5")
    tab = nabo_amd.gene_stats(fn)
    names, cols = nabo_amd._qc._table(tab)
    ref = qref.stats_of(d, "A")
    check("stats names and valid", names == ref["genes"] and np.array_equal(cols["valid_gene"], ref["valid_gene"]) and np.array_equal(cols["ncells"], ref["ncells"]))
    for k in ("m", "nzm", "variance"):
        check("stats " + k, np.allclose(cols[k], ref[k], rtol=1e-5, atol=0))          # the reference's statistics are float32
    tab, bins_min, cor = nabo_amd.correct_var(tab)
    check("bins", bins_min.shape == d["A_bins_min_100"].shape and np.allclose(bins_min, d["A_bins_min_100"], rtol=1e-5))
    with contextlib.redirect_stdout(io.StringIO()) as out:
        hv = nabo_amd.find_hvgs(tab, use_corrected_var=True, dataset_h5=fn, update_cache=True)
    check("hvgs", hv == [str(x) for x in d["A_hvg_corrected"]] and out.getvalue() == "%d highly variable genes found\n" % len(hv))
    check("hvg_list", [x.decode() for x in stored(fn, "hvg_list")] == hv)
    lvg_args = json.loads(str(d["lvg_args"]))
    check("lvgs", nabo_amd.get_lvgs(tab, hvgs=d["A_hvg_explicit"], **lvg_args["cutoff"]) == [str(x) for x in d["A_lvg_cutoff"]])
    fit = nabo_amd.fit_pca(fn, hv, n_comps=5)
    out_fn = os.path.join(td, "pca.h5")
    nabo_amd.transform_pca(fn, out_fn, "pca", fit, fit.scaling_params, layout="dense")
    import h5py
    with h5py.File(out_fn, "r") as h5:
        Z = h5["pca"]["__pca_matrix"][:]
    check("projection", Z.shape == (len(d["A_keep_cells"]), 5) and np.isfinite(Z).all() and np.abs(Z).max() > 0)
    print("RESULT " + json.dumps({"checked": checked, "differ": differ}))


if __name__ == "__main__":
    main()
