"""File-level PCA functions (nabo_amd.get_scaling_params, transform_pca) on Nabo-format dataset files written from
tests/golden/pca.npz, against what the reference computed from the same files, and `Mapping` on the groups they write
in both layouts.  Needs h5py and a GPU: run by test_pca_gpu.py under an interpreter with h5py."""
import contextlib
import io
import json
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import _pca_ref as pref  # noqa: E402
from _mapping_case import read_graph_like_reference  # noqa: E402

import nabo_amd  # noqa: E402

nabo_amd._lib.lib()          # before pandas comes in: its numexpr may bring an older libstdc++ than the library needs


def write_dataset(fn, d, prefix, with_keeps, shuffle_records=False):
    """names/{cells,genes}, gene_data/<gene> and cell_data/<cell> as (idx, val) records, processed_data/{sf,keep_*_idx}"""
    import h5py
    rec = [("idx", np.uint32), ("val", np.float32)]
    with h5py.File(fn, "w") as h5:
        g = h5.create_group("names")
        g.create_dataset("cells", data=np.array([str(x).encode() for x in d[prefix + "_cells"]]))
        g.create_dataset("genes", data=np.array([str(x).encode() for x in d[prefix + "_genes"]]))
        for grp, names, ptr, idx, val in (("gene_data", d[prefix + "_genes"], d[prefix + "_gene_ptr"], d[prefix + "_cell"], d[prefix + "_val"]),
                                          ("cell_data", d[prefix + "_cells"], d[prefix + "_cell_ptr"], d[prefix + "_gene"], d[prefix + "_cval"])):
            hg = h5.create_group(grp)
            for j, name in enumerate(names):
                r = np.zeros(int(ptr[j + 1] - ptr[j]), dtype=rec)
                r["idx"], r["val"] = idx[ptr[j]:ptr[j + 1]], val[ptr[j]:ptr[j + 1]]
                if shuffle_records:                              # the file may list a record's entries in any order
                    r = r[np.random.default_rng(j).permutation(r.shape[0])]
                hg.create_dataset(str(name), data=r)
        p = h5.create_group("processed_data")
        p.create_dataset("sf", data=d[prefix + "_sf"])
        if with_keeps:
            p.create_dataset("keep_cells_idx", data=d[prefix + "_keep_cells"])
            p.create_dataset("keep_genes_idx", data=d[prefix + "_keep_genes"])


def read_vectors(fn, grp, cells):
    import h5py
    with h5py.File(fn, "r") as h5:
        g = h5[grp]
        if "__pca_matrix" in g:
            pos = {x.decode(): i for i, x in enumerate(g["__pca_cells"][:])}
            return g["__pca_matrix"][:][[pos[c] for c in cells]]
        assert sorted(g) == sorted(cells)
        return np.array([g[c][:] for c in cells])


def same(a, b):
    return a.shape == b.shape and bool(np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64)))


def params_of(p):
    return nabo_amd._pca._params(p)


def main():
    d = np.load(os.path.join(HERE, "golden", "pca.npz"))
    out = {"differ": [], "checked": 0}

    def check(name, ok):
        out["checked"] += 1
        if not ok:
            out["differ"].append(name)
    tol, m_tol, s_tol = 4 * float(d["proj_dev"]), 4 * float(d["m_dev"]), 4 * float(d["var_dev"])
    with tempfile.TemporaryDirectory() as td:
        fn_r, fn_t = os.path.join(td, "ref.h5"), os.path.join(td, "target.h5")
        write_dataset(fn_r, d, "r", True, shuffle_records=True)
        write_dataset(fn_t, d, "t", False)
        # ---- get_scaling_params: selection, order, values
        asked = [str(x) for x in d["pca_asked"]]
        for genes, only_valid, key in ((None, True, "r_params"), (None, False, "r_params_any"), (asked, True, None)):
            names, mu, sigma = params_of(nabo_amd.get_scaling_params(fn_r, genes, only_valid))
            wn, wm, ws = (d[key + "_genes"], d[key + "_mu"], d[key + "_sigma"]) if key else (d["pca_genes"], d["pca_mu"], d["pca_sigma"])
            check("scaling params %s: genes" % key, names == [str(x) for x in wn])
            check("scaling params %s: mu" % key, bool((np.abs(mu - wm) <= m_tol * np.abs(wm)).all()))
            check("scaling params %s: sigma" % key, bool((np.abs(sigma - ws) <= s_tol * np.abs(ws)).all()))
        try:
            nabo_amd.get_scaling_params(fn_r, ["G7", "G4", "nobody"])
            check("none valid raises", False)
        except ValueError as e:
            check("none valid raises", pref.meta(d)["none_valid"] == "ValueError: " + str(e))
        # ---- transform_pca with the reference's own parameters and transformer, both layouts
        tr = types.SimpleNamespace(mean_=d["pca_mean"], components_=d["pca_components"])
        sp = nabo_amd._pca._as_params([str(x) for x in d["pca_genes"]], d["pca_mu"], d["pca_sigma"])
        calls = {name: (kw, Zref) for name, _, kw, Zref in pref.projection_calls(d)}
        fns = {}
        for layout in ("cells", "dense"):
            fns[layout] = os.path.join(td, "pca_%s.h5" % layout)
            for name, fn, fill in (("ref", fn_r, False), ("target", fn_t, True)):
                msg = io.StringIO()
                with contextlib.redirect_stdout(msg):
                    nabo_amd.transform_pca(fn, fns[layout], name, tr, sp, fill_missing=fill, layout=layout)
                    nabo_amd.transform_pca(fn, fns[layout], name, tr, sp, fill_missing=fill, layout=layout, mem_budget=6000)   # replaces the group
                kw, Zref = calls[name]
                chunks = nabo_amd._pca.last_device_ms()[1]
                cells = [str(d[("r" if name == "ref" else "t") + "_cells"][i]) for i in kw["rows"]]
                Z = read_vectors(fns[layout], name, cells)
                check("%s %s: several chunks" % (layout, name), chunks > 1)
                check("%s %s: the written vectors are pca_project_csr's" % (layout, name), same(Z, nabo_amd.pca_project_csr(**kw)))
                check("%s %s: the restatement's, bit for bit" % (layout, name), same(Z, pref.project(**kw)))
                check("%s %s: the reference's vectors" % (layout, name), pref.row_dev(Zref, Z) <= tol)
                check("%s %s: warning" % (layout, name), (msg.getvalue().strip().splitlines() or [""])[0] == (pref.meta(d)["warning"] if fill else ""))
        try:
            nabo_amd.transform_pca(fn_t, fns["cells"], "target", tr, sp)
            check("a missing gene raises", False)
        except KeyError:
            check("a missing gene raises", True)
        check("the refused call left the group alone", read_vectors(fns["cells"], "target", [str(x) for x in d["t_cells"]]).shape == d["t_Z"].shape)
        for bad in (dict(transformer=None), dict(scaling_params=None), dict(layout="rows"),
                    dict(transformer=types.SimpleNamespace(mean_=tr.mean_, components_=tr.components_, whiten=True))):
            try:
                nabo_amd.transform_pca(**dict(dict(dataset_h5=fn_r, out_file=fns["cells"], pca_group_name="x", transformer=tr, scaling_params=sp), **bad))
                check("refused: %s" % list(bad), False)
            except ValueError:
                check("refused: %s" % list(bad), True)
        print("PARTIAL " + json.dumps(out, default=str), flush=True)
        # ---- Mapping reads either layout: identical graphs
        graphs = {}
        for layout in ("cells", "dense"):
            map_fn = os.path.join(td, "mapping_%s.h5" % layout)
            with contextlib.redirect_stdout(io.StringIO()):
                m = nabo_amd.Mapping(map_fn, "WT", fns[layout], "ref", overwrite=True)
                m.set_parameters(8, 11, 0.25, 100)
                m.make_ref_graph()
                m.map_target("T", fns[layout], "target")
            rn, re_, _ = read_graph_like_reference(map_fn, "WT", "reference")
            tn, te, _ = read_graph_like_reference(map_fn, "T", "target")
            graphs[layout] = (rn, re_, tn, te)
            check("%s: graph sizes" % layout, len(rn) == len(d["r_keep_cells"]) and len(re_) > len(rn) and len(te) > 200)
        check("both layouts give the same graphs", graphs["cells"] == graphs["dense"])
        out["ref_edges"], out["target_edges"] = len(graphs["cells"][1]), len(graphs["cells"][3])
    print("RESULT " + json.dumps(out, default=str))


if __name__ == "__main__":
    main()
