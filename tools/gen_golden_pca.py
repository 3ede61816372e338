#!/opt/conda/bin/python3.9
"""Golden vectors for the PCA projection and the gene statistics of the reference (nabo/_dataset.py): set_gene_stats
(:594-637), get_scaling_params (:814-844), get_scaled_values (:846-915), fit_ipca (:917-983), transform_pca (:985-1033).

TEST INFRASTRUCTURE ONLY, run where the reference is mounted, with an interpreter that has h5py, pandas and sklearn:

    /opt/conda/bin/python3.9 tools/gen_golden_pca.py

The reference's nabo/_dataset.py is loaded BY FILE PATH under a stub `nabo` package (as tools/gen_golden_de.py does).
Seeded synthetic datasets are written as Nabo-format HDF5 files into a temporary directory -- a reference sample of
300 cells x 120 genes with a keep_cells_idx that drops cells, a keep_genes_idx that drops genes, kept genes without a
nonzero value and stored size factors; a target sample of 200 cells holding most of the same genes in another order
plus a few others -- the reference's own functions run on them, and only DATA goes to tests/golden/pca.npz: the sparse
inputs in both orientations, the gene statistics, mu and sigma, mean_ and components_, every projected vector.

Measured values are stored with them, against the tests' restatement (tests/_pca_ref.py); no test hard-codes them:
  proj_dev                 the largest ||reference row - restated row||inf / max(1, ||reference row||inf): the reference
                           rounds ((x - mu) / sigma - mean) per gene and multiplies through BLAS in another order;
  m_dev, nzm_dev, var_dev  the largest relative differences between the reference's float32 statistics and the
                           restatement's float64 ones.
The script asserts that the scaled vectors the reference yields are float64 and that proj_dev is below 1e-9.
"""
import contextlib
import importlib.util
import io
import json
import os
import sys
import tempfile
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
REF = os.environ.get("NABO_REFERENCE", "/root/reference")
GOLD = os.path.join(REPO, "tests", "golden")
sys.path.insert(0, os.path.join(REPO, "tests"))
import _pca_ref as pref  # noqa: E402


def load_reference():
    nb = types.ModuleType("numba")
    nb.jit = lambda *a, **k: (a[0] if len(a) == 1 and callable(a[0]) and not k else (lambda f: f))
    sys.modules["numba"] = nb
    pkg = types.ModuleType("nabo")
    pkg.__path__ = []
    sys.modules["nabo"] = pkg
    spec = importlib.util.spec_from_file_location("nabo._dataset", os.path.join(REF, "nabo", "_dataset.py"))
    m = importlib.util.module_from_spec(spec)
    sys.modules["nabo._dataset"] = m
    spec.loader.exec_module(m)
    return m


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()) as out, contextlib.redirect_stderr(io.StringIO()), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        r = fn(*a, **k)
    quiet.last = out.getvalue()
    return r


def synth(rng, n_cells, n_genes, density, empty=(), only_in=None):
    """a cells x genes matrix of counts, dense in memory (it is small): gene j is expressed in about density * (1 + j % 5)
    of the cells; genes in `empty` nowhere; only_in = (gene, cells): that gene in those cells alone"""
    p = np.minimum(1.0, density * (1 + np.arange(n_genes) % 5))[None, :]
    X = np.where(rng.random((n_cells, n_genes)) < p, rng.poisson(1.5 + np.arange(n_genes) % 7, (n_cells, n_genes)) + 1, 0).astype(np.float32)
    for j in empty:
        X[:, j] = 0
    if only_in is not None:
        X[:, only_in[0]] = 0
        X[only_in[1], only_in[0]] = 3
    return X


def write_dataset(fn, cells, genes, X, sf, keep_cells_idx, keep_genes_idx):
    import h5py
    with h5py.File(fn, "w") as h5:
        g = h5.create_group("names")
        g.create_dataset("cells", data=np.array([x.encode() for x in cells]))
        g.create_dataset("genes", data=np.array([x.encode() for x in genes]))
        rec = [("idx", np.uint32), ("val", np.float32)]
        gd, cd = h5.create_group("gene_data"), h5.create_group("cell_data")
        for j, name in enumerate(genes):
            idx = np.nonzero(X[:, j])[0]
            d = np.zeros(len(idx), dtype=rec)
            d["idx"], d["val"] = idx, X[idx, j]
            gd.create_dataset(name, data=d)
        for i, name in enumerate(cells):
            idx = np.nonzero(X[i])[0]
            d = np.zeros(len(idx), dtype=rec)
            d["idx"], d["val"] = idx, X[i, idx]
            cd.create_dataset(name, data=d)
        p = h5.create_group("processed_data")
        p.create_dataset("sf", data=sf)
        if keep_cells_idx is not None:
            p.create_dataset("keep_cells_idx", data=np.array(keep_cells_idx))
        if keep_genes_idx is not None:
            p.create_dataset("keep_genes_idx", data=np.array(keep_genes_idx))


def store(out, prefix, cells, genes, X, sf, keep_cells_idx, keep_genes_idx):
    out[prefix + "_cells"], out[prefix + "_genes"] = np.array(cells), np.array(genes)
    ci, gi = np.nonzero(X)                                       # cell-major: compressed sparse rows
    out[prefix + "_cell_ptr"] = np.concatenate([[0], np.cumsum(np.bincount(ci, minlength=len(cells)))]).astype(np.int64)
    out[prefix + "_gene"], out[prefix + "_cval"] = gi.astype(np.int32), X[ci, gi].astype(np.float32)
    gj, cj = np.nonzero(X.T)                                     # gene-major: compressed sparse columns
    out[prefix + "_gene_ptr"] = np.concatenate([[0], np.cumsum(np.bincount(gj, minlength=len(genes)))]).astype(np.int64)
    out[prefix + "_cell"], out[prefix + "_val"] = cj.astype(np.int32), X[cj, gj].astype(np.float32)
    out[prefix + "_sf"] = sf
    out[prefix + "_keep_cells"] = np.arange(len(cells), dtype=np.int64) if keep_cells_idx is None else np.array(keep_cells_idx, dtype=np.int64)
    out[prefix + "_keep_genes"] = np.arange(len(genes), dtype=np.int64) if keep_genes_idx is None else np.array(keep_genes_idx, dtype=np.int64)


def read_group(fn, grp, cells):
    import h5py
    with h5py.File(fn, "r") as h5:
        assert sorted(h5[grp]) == sorted(cells)
        return np.array([h5[grp][c][:] for c in cells], dtype=np.float64)


def main():
    ds_mod = load_reference()
    rng = np.random.default_rng(20240923)
    out = {}
    td = tempfile.mkdtemp()

    # ---- the reference sample: 300 cells x 120 genes
    cells_r = ["r%d" % i for i in range(300)]
    genes_r = ["G%d" % i for i in range(120)]
    keep_cells_r = [i for i in range(300) if i % 11 != 3]
    keep_genes_r = [i for i in range(120) if i % 9 != 4]
    dropped = [i for i in range(300) if i % 11 == 3]
    # G7 (kept) has no nonzero at all, G20 (kept) only in cells keep_cells_idx drops: both are invalid genes
    Xr = synth(rng, 300, 120, 0.08, empty=(7,), only_in=(20, dropped[:5]))
    sf_r = (0.5 + rng.random(300) * 1.5).astype(np.float32)
    fn_r = os.path.join(td, "ref.h5")
    write_dataset(fn_r, cells_r, genes_r, Xr, sf_r, keep_cells_r, keep_genes_r)
    store(out, "r", cells_r, genes_r, Xr, sf_r, keep_cells_r, keep_genes_r)
    # ---- the target sample: 200 cells, 100 of the reference's genes in another order and 8 others
    cells_t = ["t%d" % i for i in range(200)]
    genes_t = [genes_r[i] for i in rng.permutation(120)[:100]] + ["H%d" % i for i in range(8)]
    Xt = synth(rng, 200, 108, 0.10)
    Xt[5] = 0                                                    # a cell without any entry
    sf_t = (0.5 + rng.random(200) * 1.5).astype(np.float32)
    fn_t = os.path.join(td, "target.h5")
    write_dataset(fn_t, cells_t, genes_t, Xt, sf_t, None, None)
    store(out, "t", cells_t, genes_t, Xt, sf_t, None, None)

    ds_r, ds_t = quiet(ds_mod.Dataset, fn_r), quiet(ds_mod.Dataset, fn_t)
    assert list(ds_r.keepCellsIdx) == keep_cells_r and list(ds_r.keepGenesIdx) == keep_genes_r and ds_r.sf.dtype == np.float32

    # ---- set_gene_stats, get_scaling_params
    quiet(ds_r.set_gene_stats)
    gs = ds_r.geneStats
    assert list(gs.index) == genes_r
    valid = np.array([bool(x) for x in gs.valid_gene.values])
    assert not valid[7] and not valid[20] and not valid[4] and valid[keep_genes_r].sum() == len(keep_genes_r) - 2
    assert gs.m.dtype == np.float64 and gs.variance.dtype == np.float64, (gs.m.dtype, gs.variance.dtype)
    stats = {"valid": valid.astype(np.uint8), "ncells": np.where(valid, gs.ncells.values.astype(np.float64), 0).astype(np.int64)}
    for k in ("m", "nzm", "variance"):
        stats[k] = np.where(valid, gs[k].values.astype(np.float64), 0.0)
    for k, v in stats.items():
        out["r_stats_" + k] = v
    sp_all = quiet(ds_r.get_scaling_params)
    out["r_params_genes"], out["r_params_mu"], out["r_params_sigma"] = np.array(list(sp_all.index)), sp_all["mu"].values, sp_all["sigma"].values
    assert list(sp_all.index) == [g for g, v in zip(genes_r, valid) if v]
    sp_any = quiet(ds_r.get_scaling_params, None, False)        # only_valid=False: invalid genes carry the columns' minima
    out["r_params_any_genes"], out["r_params_any_mu"], out["r_params_any_sigma"] = np.array(list(sp_any.index)), sp_any["mu"].values, sp_any["sigma"].values
    try:
        quiet(ds_r.get_scaling_params, ["G7", "G4", "nobody"])
        none_valid = "ok"
    except ValueError as e:
        none_valid = "ValueError: " + str(e)
    restated = pref.gene_stats(*pref.csc_of(out, "r"), keep_cells=keep_cells_r, keep_genes=pref.keep_mask(out, "r"))
    assert np.array_equal(restated["valid"], stats["valid"]) and np.array_equal(restated["ncells"], stats["ncells"])
    m_dev, nzm_dev, var_dev = pref.stats_devs(stats, restated)

    # ---- fit_ipca on 40 genes (given out of file order, with an invalid and an unknown one among them), 8 components
    asked = [genes_r[i] for i in rng.permutation(120)[:46]]
    asked = [g for g in asked if g not in ("G7", "G20")][:40] + ["G7", "nobody"]
    quiet(ds_r.fit_ipca, asked, 8, None, True)
    sp = quiet(ds_r.get_scaling_params, asked)
    sel = list(sp.index)
    assert sel == ds_r.ipca.genes and sel == [g for g in asked if g in set(sp_all.index)] and 30 <= len(sel) <= 40
    out["pca_asked"], out["pca_genes"] = np.array(asked), np.array(sel)
    out["pca_mu"], out["pca_sigma"] = sp["mu"].values.astype(np.float64), sp["sigma"].values.astype(np.float64)
    assert sp["mu"].values.dtype == np.float64 and sp["sigma"].values.dtype == np.float64
    out["pca_mean"], out["pca_components"] = ds_r.ipca.mean_.astype(np.float64), ds_r.ipca.components_.astype(np.float64)
    assert ds_r.ipca.components_.shape == (8, len(sel)) and not ds_r.ipca.whiten

    # ---- the scaled vectors are float64; transform_pca of both samples
    for ds, fill in ((ds_r, False), (ds_t, True)):
        for _, a in quiet(lambda: list(ds.get_scaled_values(sp, disable_tqdm=True, fill_missing=fill))):
            assert a.dtype == np.float64, a.dtype
    fn_out = os.path.join(td, "pca.h5")
    quiet(ds_r.transform_pca, fn_out, "ref_pca", ds_r.ipca, sp, True)
    out["r_Z"] = read_group(fn_out, "ref_pca", [cells_r[i] for i in keep_cells_r])
    try:
        quiet(ds_t.transform_pca, fn_out, "target_pca", ds_r.ipca, sp, True, False)
        key_error = "ok"
    except KeyError:
        key_error = "KeyError"
    assert key_error == "KeyError"
    quiet(ds_t.transform_pca, fn_out, "target_pca", ds_r.ipca, sp, True, True)
    warning = quiet.last.strip()
    out["t_Z"] = read_group(fn_out, "target_pca", cells_t)
    n_missing = len([g for g in sel if g not in set(genes_t)])
    assert n_missing >= 2 and warning == "WARNING: %d out %d genes are missing in this dataset" % (n_missing, len(sel)), warning

    # ---- the restatement against the reference's vectors
    proj_dev = 0.0
    for name, prefix, kw, Zref in pref.projection_calls(out):
        Z = pref.project(**kw)
        dev = pref.row_dev(Zref, Z)
        print("  %-8s %4d rows x %d, deviation %.3g" % (name, Z.shape[0], Z.shape[1], dev))
        proj_dev = max(proj_dev, dev)
    assert 0 < proj_dev < 1e-9, proj_dev
    out["proj_dev"], out["m_dev"], out["nzm_dev"], out["var_dev"] = (np.float64(x) for x in (proj_dev, m_dev, nzm_dev, var_dev))
    out["meta"] = np.array(json.dumps({"fill_missing_false": key_error, "warning": warning, "n_missing": n_missing, "none_valid": none_valid}))
    fn = os.path.join(GOLD, "pca.npz")
    np.savez_compressed(fn, **out)
    print("proj_dev %.3g, m_dev %.3g, nzm_dev %.3g, var_dev %.3g" % (proj_dev, m_dev, nzm_dev, var_dev))
    print("wrote %s (%d bytes)" % (fn, os.path.getsize(fn)))


if __name__ == "__main__":
    sys.exit(main())
