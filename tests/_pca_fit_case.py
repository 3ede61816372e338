"""File-level PCA fit (nabo_amd.fit_pca) on a Nabo-format dataset file written from tests/golden/pca_fit.npz, then
transform_pca with the result and `Mapping.make_ref_graph` on what it wrote.  Needs h5py and a GPU: run by
test_pca_fit_gpu.py under an interpreter with h5py."""
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
import _pca_fit_ref as fref  # noqa: E402
from _mapping_case import read_graph_like_reference  # noqa: E402
from _pca_case import read_vectors, same, write_dataset  # noqa: E402

import nabo_amd  # noqa: E402

nabo_amd._lib.lib()          # before pandas comes in: its numexpr may bring an older libstdc++ than the library needs


def with_columns(d):
    """the golden's rows of cells in the layout _pca_case.write_dataset reads, with the columns of genes derived from them"""
    n_cells, n_genes = len(d["cells"]), len(d["genes"])
    cell_of = np.repeat(np.arange(n_cells), np.diff(d["cell_ptr"]))
    order = np.lexsort((cell_of, d["gene"]))
    return {"s_cells": d["cells"], "s_genes": d["genes"], "s_cell_ptr": d["cell_ptr"], "s_gene": d["gene"], "s_cval": d["cval"], "s_sf": d["sf"],
            "s_gene_ptr": np.concatenate([[0], np.cumsum(np.bincount(d["gene"], minlength=n_genes))]).astype(np.int64),
            "s_cell": cell_of[order].astype(np.int32), "s_val": d["cval"][order], "s_keep_cells": d["keep_cells"], "s_keep_genes": d["keep_genes"]}


def main():
    d = np.load(os.path.join(HERE, "golden", "pca_fit.npz"))
    out = {"differ": [], "checked": 0}

    def check(name, ok):
        out["checked"] += 1
        if not ok:
            out["differ"].append(name)
    with tempfile.TemporaryDirectory() as td:
        fn = os.path.join(td, "sample.h5")
        write_dataset(fn, with_columns(d), "s", True)
        asked = [str(x) for x in d["trunc_asked"]]
        msg = io.StringIO()
        with contextlib.redirect_stdout(msg):
            fit = nabo_amd.fit_pca(fn, asked, n_comps=10, batch_size=7)
        names, mu, sigma = nabo_amd._pca._params(fit.scaling_params)
        check("genes", fit.genes == names == [str(x) for x in d["trunc_genes"]])
        check("no warning", msg.getvalue() == "")
        check("mu, sigma", bool(np.allclose(mu, d["trunc_mu"], rtol=1e-5, atol=0) and np.allclose(sigma, d["trunc_sigma"], rtol=1e-5, atol=0)))
        check("shapes", fit.components_.shape == (10, len(names)) and fit.n_samples_seen_ == len(d["keep_cells"]) and fit.n_components_ == 10)
        # the same fit through the arrays, with the file's own scaling parameters: bit for bit
        kw, _ = fref.fit_call(d, "trunc")
        arr = nabo_amd.fit_pca_csr(n_comps=10, **dict(kw, mu=mu, sigma=sigma))
        check("fit_pca is fit_pca_csr on the file's arrays", same(fit.components_, arr.components_) and same(fit.mean_, arr.mean_)
              and same(fit.explained_variance_, arr.explained_variance_))
        # n_comps above the number of asked genes: the reference's reset and warning
        msg = io.StringIO()
        with contextlib.redirect_stdout(msg):
            fit5 = nabo_amd.fit_pca(fn, asked[:5], n_comps=9)
        check("reset to the number of features", fit5.components_.shape == (5, 5)
              and msg.getvalue().strip() == "WARNING: Number of components were reset to number of features i.e. 5")
        # transform_pca takes the result unchanged; the vectors are the fit's own transform of the scaled cells
        pca_fn = os.path.join(td, "pca.h5")
        nabo_amd.transform_pca(fn, pca_fn, "ref", fit, fit.scaling_params)
        cells = [str(d["cells"][i]) for i in d["keep_cells"]]
        Z = read_vectors(pca_fn, "ref", cells)
        Y = fref.scaled_rows(**dict(kw, mu=mu, sigma=sigma))
        check("vector shape", Z.shape == (len(cells), 10))
        check("vectors are the fit's transform", fref.row_dev(fit.transform(Y), Z) <= 1e-12)
        check("the vectors' variances are the explained variances", bool(np.allclose(Z.var(axis=0, ddof=1), fit.explained_variance_, rtol=1e-9)))
        check("centred", bool(np.abs(Z.mean(axis=0)).max() <= 1e-12))
        map_fn = os.path.join(td, "mapping.h5")
        with contextlib.redirect_stdout(io.StringIO()):
            m = nabo_amd.Mapping(map_fn, "WT", pca_fn, "ref", overwrite=True)
            m.set_parameters(8, 11, 0.25, 100)
            m.make_ref_graph()
        rn, re_, _ = read_graph_like_reference(map_fn, "WT", "reference")
        check("graph sizes", len(rn) == len(cells) and len(re_) > len(rn))
        out["ref_edges"] = len(re_)
    print("RESULT " + json.dumps(out, default=str))


if __name__ == "__main__":
    main()
