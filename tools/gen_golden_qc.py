#!/opt/conda/bin/python3.9
"""Golden vectors for the quality-control step of the reference (nabo/_dataset.py): filter_data (:342-425), set_sf
(:548-592), set_gene_stats (:594-637), correct_var (:639-683), find_hvgs (:685-755) and get_lvgs (:772-812).

TEST INFRASTRUCTURE ONLY, run where the reference is mounted, with an interpreter that has h5py, pandas and statsmodels:

    /opt/conda/bin/python3.9 tools/gen_golden_qc.py

The reference's nabo/_dataset.py is loaded BY FILE PATH under a stub `nabo` package (as tools/gen_golden_pca.py does),
with a stand-in `nabo._plotting` whose plot_mean_var does nothing (find_hvgs imports it unconditionally).  Seeded
synthetic datasets of 400 cells x 600 genes are written as Nabo-format HDF5 files into a temporary directory, the
reference's own functions run on them, and only DATA goes to tests/golden/qc.npz.

Sample A: integer counts, gene means spread over decades.  Among the names: MT- and RPS/RPL/MRPS/MRPL genes, a lower-case
`mt-x` whose upper-case form the file lacks, a lower-case `mito_a` whose upper-case form is another gene, an all-zero
gene, an empty cell, and thresholds every one of the eight cell criteria removes cells by; run once without keep lists in
the file and once with.  Sample B: the same pattern with non-integer values, thresholds placed in gaps.

Measured and stored, never hard-coded in a test:
  tot_dev        sample B, the largest relative difference of the header's float64 sums from the reference's float32 ones;
  lowess_dev     nabo_amd._qc.lowess against statsmodels on the bins' values, largest |difference| / max(1, |value|);
  fixed_var_dev  nabo_amd._qc.correct_var fed the reference's statistics against its fixed_var, largest relative one.
Asserted, so that the tests can demand equality: on sample A tests/_qc_ref.py reproduces every keep list, report count
and size-factor bit; the HVG and LVG lists from the restated float64 statistics (tests/_pca_ref.gene_stats) equal the
reference's; no log-mean lies within 1e-9 (relative) of an interior bin edge; no two genes tie in the LVG sort; in
sample B no value lies within 1000 x tot_dev of its threshold.  If a seed breaks a condition, change the seed.
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
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
REF = os.environ.get("NABO_REFERENCE", "/root/reference")
GOLD = os.path.join(REPO, "tests", "golden")
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, REPO)
import _pca_ref as pref  # noqa: E402
import _qc_ref as qref  # noqa: E402

SEED = 20241018
MITO_PATTERNS = ["^MT-", "^mt-", "^mito_"]
RIBO_PATTERNS = ["^RPS", "^RPL", "^MRPS", "^MRPL"]
SPECIAL = {3: "MT-A", 50: "MT-B", 120: "MT-C", 7: "RPS1", 90: "RPL2", 200: "MRPS3", 310: "MRPL4", 33: "mt-x", 400: "mito_a", 401: "MITO_A"}
ZERO_GENE, EMPTY_CELL = 11, 5
BURST_GENES = range(150, 158)


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


def synth(rng, n_cells=400, n_genes=600):
    lam = 10.0 ** rng.uniform(-2.5, 1.0, n_genes)
    for j, name in SPECIAL.items():
        lam[j] = 2.0 + 3.0 * rng.random()
    depth = rng.lognormal(0.0, 0.6, n_cells)
    X = rng.poisson(lam[None, :] * depth[:, None]).astype(np.float32)
    mito = [j for j, g in SPECIAL.items() if g.upper().startswith(("MT-", "MITO_"))]
    ribo = [j for j, g in SPECIAL.items() if g.startswith(("RPS", "RPL", "MRPS", "MRPL"))]
    X[np.ix_(range(20, 24), mito)] = 0                  # no mito expression at all
    X[np.ix_(range(30, 33), mito)] *= 25
    X[np.ix_(range(40, 44), ribo)] = 0
    X[np.ix_(range(50, 53), ribo)] *= 25
    for j in BURST_GENES:                               # rare and strong: variance / mean above the other genes' variances
        X[:, j] = rng.poisson(0.06 * depth)
        X[rng.choice(np.arange(60, n_cells), 4, replace=False), j] += 200
    X[:, ZERO_GENE] = 0
    X[EMPTY_CELL] = 0
    genes = [SPECIAL.get(j, "G%d" % j) for j in range(n_genes)]
    return ["c%d" % i for i in range(n_cells)], genes, X


def write_dataset(fn, cells, genes, X, keep_cells_idx=None, keep_genes_idx=None):
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
        if keep_cells_idx is not None:
            p = h5.create_group("processed_data")
            p.create_dataset("keep_cells_idx", data=np.array(keep_cells_idx))
            p.create_dataset("keep_genes_idx", data=np.array(keep_genes_idx))


def gap(values, q, margin):
    """a threshold near the q-quantile of the finite values, in the middle of a gap at least 2 * margin (relative) wide"""
    v = np.unique(np.asarray(values, dtype=np.float64)[np.isfinite(values)])
    i = max(1, int(q * v.shape[0]))
    while i < v.shape[0] and not (v[i] - v[i - 1]) / 2 > margin * abs(v[i]):
        i += 1
    assert i < v.shape[0], "no gap wide enough"
    return float((v[i] + v[i - 1]) / 2)


def counts_of(text):
    lines = [ln for ln in text.splitlines() if "filtered" in ln]
    assert len(lines) == 4 and lines[0].startswith("UMI filtered  : Low:"), text
    out = []
    for ln in lines:
        w = ln.split()
        out += [int(w[w.index("Low:") + 1]), int(w[w.index("High:") + 1])]
    return out, lines


def run_filter(ds_mod, td, tag, cells, genes, X, thr, pre=None):
    fn = os.path.join(td, tag + ".h5")
    write_dataset(fn, cells, genes, X, *(pre or (None, None)))
    ds = quiet(ds_mod.Dataset, fn, MITO_PATTERNS, RIBO_PATTERNS)
    quiet(ds.filter_data, **thr)
    counts, lines = counts_of(quiet.last)
    return ds, fn, counts, lines


def save_npz(fn, out):
    """np.savez_compressed with a fixed time stamp per member: the same data gives the same bytes"""
    with zipfile.ZipFile(fn, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(out):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(out[k]), allow_pickle=False)
            zi = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            zi.external_attr = 0o644 << 16
            z.writestr(zi, buf.getvalue())


def main():
    from nabo_amd import _qc
    from statsmodels.nonparametric.smoothers_lowess import lowess as sm_lowess
    ds_mod = load_reference()
    rng = np.random.default_rng(SEED)
    td = tempfile.mkdtemp()
    out = {}
    cells, genes, XA = synth(rng)
    # sample B: the same pattern as from a normalised table, values on a grid of 2^-16
    fac = (0.3 + rng.random(XA.shape[0]))[:, None] * (0.5 + rng.random(XA.shape[1]))[None, :]
    XB = (np.round(XA * fac * 65536) / 65536).astype(np.float32)
    XB[XA > 0] = np.maximum(XB[XA > 0], np.float32(1 / 65536))
    n_cells, n_genes = XA.shape
    pre_cells = [i for i in range(n_cells) if i % 7 != 2]
    pre_genes = [i for i in range(n_genes) if i % 9 != 4]
    out["genes"], out["cells"] = np.array(genes), np.array(cells)
    out["pre_cells"], out["pre_genes"] = np.array(pre_cells, dtype=np.int64), np.array(pre_genes, dtype=np.int64)
    tot_dev = 0.0

    for s, X in (("A", XA), ("B", XB)):
        ci, gi = np.nonzero(X)
        cell_ptr = np.concatenate([[0], np.cumsum(np.bincount(ci, minlength=n_cells))]).astype(np.int64)
        gene, val = gi.astype(np.int32), X[ci, gi].astype(np.float32)
        if s == "A":
            out["cell_ptr"], out["gene"] = cell_ptr, gene       # both samples list the same entries
        else:
            assert np.array_equal(out["cell_ptr"], cell_ptr) and np.array_equal(out["gene"], gene)
        out[s + "_val"] = val
        fn0 = os.path.join(td, s + "_probe.h5")
        write_dataset(fn0, cells, genes, X)
        ds = quiet(ds_mod.Dataset, fn0, MITO_PATTERNS, RIBO_PATTERNS)
        assert "mt-x" in ds.mitoGenes and "mito_a" in ds.mitoGenes and "MITO_A" not in ds.mitoGenes and "RPS1" in ds.riboGenes
        tot, ng = quiet(ds.get_total_exp_per_cell), quiet(ds.get_genes_per_cell)
        cm, cr, ab = quiet(ds.get_cum_exp, ds.mitoGenes), quiet(ds.get_cum_exp, ds.riboGenes), quiet(ds.get_gene_abundance)
        assert tot.dtype == np.float32 and cm.dtype == np.float32
        with np.errstate(all="ignore"):
            pm, pr = 100 * cm / tot, 100 * cr / tot
        assert pm.dtype == np.float32 and np.isnan(pm[EMPTY_CELL])
        out[s + "_tot"], out[s + "_ngenes"], out[s + "_cum_mito"], out[s + "_cum_ribo"] = tot, ng, cm, cr
        out[s + "_pct_mito"], out[s + "_pct_ribo"], out[s + "_abundance"] = pm, pr, ab.astype(np.int64)
        cls = qref.class_bits(genes, MITO_PATTERNS, RIBO_PATTERNS)
        n_ent, sums = qref.cell_qc(cell_ptr, gene, val, cls, 2)
        assert np.array_equal(n_ent, ng.astype(np.int64))
        if s == "A":
            assert tot.max() < 2 ** 24 and np.array_equal(sums.astype(np.float32), np.stack([tot, cm, cr], axis=1))
            thr = dict(min_exp=int(np.quantile(tot, 0.10)), max_exp=int(np.quantile(tot, 0.97)), min_ngenes=int(np.quantile(ng, 0.06)),
                       max_ngenes=int(np.quantile(ng, 0.98)), min_mito=0.01, max_mito=float(np.float32(np.nanquantile(pm, 0.97))),
                       min_ribo=0.01, max_ribo=float(np.float32(np.nanquantile(pr, 0.97))), min_gene_abundance=10)
        else:
            ref3 = np.stack([tot, cm, cr], axis=1).astype(np.float64)
            nz = ref3 != 0
            tot_dev = float((np.abs(sums - ref3)[nz] / ref3[nz]).max())
            assert 0 < tot_dev < 1e-6, tot_dev
            mg = 1000 * tot_dev
            thr = dict(min_exp=gap(tot, 0.10, mg), max_exp=gap(tot, 0.97, mg), min_ngenes=int(np.quantile(ng, 0.06)) + 0.5,
                       max_ngenes=int(np.quantile(ng, 0.98)) + 0.5, min_mito=gap(pm, 0.03, mg), max_mito=gap(pm, 0.97, mg),
                       min_ribo=gap(pr, 0.03, mg), max_ribo=gap(pr, 0.97, mg), min_gene_abundance=10)
            for v, keys in ((tot, ("min_exp", "max_exp")), (pm, ("min_mito", "max_mito")), (pr, ("min_ribo", "max_ribo"))):
                for k in keys:
                    f = v[np.isfinite(v)].astype(np.float64)
                    assert (np.abs(f - thr[k]) > mg * np.abs(f)).all(), k
        out[s + "_thresholds"] = np.array(json.dumps(thr))
        for tag, pre in (("", None), ("_pre", (pre_cells, pre_genes))):
            ds, fn, counts, lines = run_filter(ds_mod, td, s + tag, cells, genes, X, thr, pre)
            assert min(counts) >= 1, counts
            kc, kg = np.array(ds.keepCellsIdx), np.array(ds.keepGenesIdx)
            assert kc.dtype == np.int64 and kg.dtype == np.int64
            out[s + tag + "_keep_cells"], out[s + tag + "_keep_genes"], out[s + tag + "_counts"] = kc, kg, np.array(counts, dtype=np.int64)
            out[s + tag + "_report"] = np.array(lines)
            got = qref.filter_ref(genes, n_ent, sums, ab, pre[0] if pre else range(n_cells), pre[1] if pre else range(n_genes),
                                  MITO_PATTERNS, RIBO_PATTERNS, thr)
            assert np.array_equal(got[0], kc) and np.array_equal(got[1], kg) and got[2] == counts, (s, tag)
            where = {g: i for i, g in enumerate(genes)}
            assert where["mito_a"] not in kg and where["mt-x"] not in kg and (where["MITO_A"] in kg) == (pre is None or where["MITO_A"] in pre[1])
            reloaded = quiet(ds_mod.Dataset, fn, MITO_PATTERNS, RIBO_PATTERNS)
            assert "INFO: Cached filtered cells loaded" in quiet.last and np.array_equal(reloaded.keepCellsIdx, kc)
            # size factors over the kept genes, over all genes, and with a size_scale float32 does not hold
            kept_cls = np.zeros(n_genes, np.uint8)
            kept_cls[kg] = 1
            _, ksum = qref.cell_qc(cell_ptr, gene, val, kept_cls, 1)
            for name, kw, col, scale in (("sf", {}, 1, 1000.0), ("sf_all", {"all_genes": True}, 0, 1000.0),
                                         ("sf_scale", {"size_scale": 1234.567}, 1, 1234.567)):
                quiet(ds.set_sf, **kw)
                assert ds.sf.dtype == np.float32
                out[s + tag + "_" + name] = ds.sf.copy()
                if s == "A":
                    assert np.array_equal(qref.sf_ref(ksum[:, col], scale).view(np.int32), ds.sf.view(np.int32)), (name, tag)
            if s == "A" and pre is None:
                dsA, fnA, kcA, kgA = ds, fn, kc, kg
    quiet(dsA.set_sf)
    sfA = dsA.sf.copy()
    assert np.array_equal(sfA, out["A_sf"])

    # ---- the statistics table, correct_var, find_hvgs, get_lvgs on sample A
    quiet(dsA.set_gene_stats)
    gs = dsA.geneStats
    assert list(gs.index) == genes
    valid = np.array([bool(x) for x in gs.valid_gene.values])
    out["A_stats_valid"] = valid.astype(np.uint8)
    for k in ("m", "nzm", "variance", "ncells"):
        out["A_stats_" + k] = gs[k].values.astype(np.float64)
    assert not valid[ZERO_GENE] and out["A_stats_ncells"][ZERO_GENE] == 0 and out["A_stats_m"][ZERO_GENE] == out["A_stats_m"][valid].min()
    # the restated float64 statistics, as a table
    gj, cj = np.nonzero(XA.T)
    csc = (np.concatenate([[0], np.cumsum(np.bincount(gj, minlength=n_genes))]).astype(np.int64), cj.astype(np.int32), XA[cj, gj].astype(np.float32), sfA)
    keep_mask = np.zeros(n_genes, np.uint8)
    keep_mask[kgA] = 1
    st = pref.gene_stats(*csc, keep_cells=kcA, keep_genes=keep_mask)
    assert np.array_equal(st["valid"], out["A_stats_valid"]) and np.array_equal(st["ncells"], out["A_stats_ncells"].astype(np.int64))
    restated = _qc._table(_qc._stats_table(genes, st))[1]
    restated = dict(restated, genes=genes)
    ref_tab = qref.stats_of(out, "A")
    lowess_dev = fixed_var_dev = 0.0
    for nb in (100, 30):
        quiet(dsA.correct_var, nb)
        fv = dsA.geneStats.fixed_var.values.astype(np.float64)
        out["A_fixed_var_%d" % nb], out["A_bins_min_%d" % nb], out["A_var_cor_%d" % nb] = fv, np.array(dsA.geneBinsMin), np.array(dsA.varCorrectionFactor)
        tab, bins_min, cor = _qc.correct_var(ref_tab, nb)
        assert np.array_equal(bins_min, dsA.geneBinsMin), nb
        mine = _qc._table(tab)[1]["fixed_var"]
        fixed_var_dev = max(fixed_var_dev, float((np.abs(mine - fv) / fv).max()))
        # the bins' (variance, mean) points, and both LOWESS curves through them
        lm, lv = np.log(out["A_stats_m"][valid]), np.log(out["A_stats_variance"][valid])
        edges = np.histogram(lm, bins=nb)[1]
        assert (np.abs(lm[:, None] - edges[None, 1:-1]) > 1e-9 * np.abs(lm[:, None])).all(), "a log-mean on a bin edge"
        pts_v = np.array([lv[np.nonzero(lm == b)[0][0]] for b in bins_min])
        theirs = sm_lowess(pts_v, bins_min, frac=0.4, it=100, return_sorted=False)
        assert np.array_equal(theirs, dsA.varCorrectionFactor)
        lowess_dev = max(lowess_dev, float((np.abs(_qc.lowess(pts_v, bins_min, 0.4, 100) - theirs) / np.maximum(1.0, np.abs(theirs))).max()))
    assert lowess_dev < 1e-9 and fixed_var_dev < 1e-9, (lowess_dev, fixed_var_dev)
    quiet(dsA.correct_var, 100)
    ref_tab = qref.stats_of(out, "A", 100)
    mine_tab = dict(_qc._table(_qc.correct_var(restated, 100)[0])[1], genes=genes)
    lg = {k: np.log(ref_tab[k][valid]) for k in ("nzm", "fixed_var")}
    explicit = dict(var_min_thresh=float(np.percentile(lg["fixed_var"], 80)), nzm_min_thresh=float(np.percentile(lg["nzm"], 20)),
                    var_max_thresh=float(np.percentile(lg["fixed_var"], 99.5)), nzm_max_thresh=float(np.percentile(lg["nzm"], 99)), min_cells=20)
    out["hvg_explicit_args"] = np.array(json.dumps(explicit))
    for name, kw in (("corrected", dict(use_corrected_var=True)), ("plain", dict(use_corrected_var=False)),
                     ("explicit", dict(use_corrected_var=True, **explicit))):
        quiet(dsA.find_hvgs, plot=False, **kw)
        hv = [str(x) for x in dsA.hvgList]
        assert 5 <= len(hv) < 200, (name, len(hv))
        out["A_hvg_" + name] = np.array(hv)
        for what, tab in (("the reference's statistics", ref_tab), ("the restated statistics", mine_tab)):
            assert quiet(_qc.find_hvgs, tab, **kw) == hv, (name, what)
    n_hvg = len(out["A_hvg_explicit"])
    nzm_cut = float(np.percentile(ref_tab["nzm"][valid], 40))
    lvg_args = {"cutoff": dict(nzm_cutoff=nzm_cut, use_corrected_var=True), "log_cutoff": dict(log_nzm_cutoff=float(np.log(nzm_cut)) + 0.25, n=25)}
    out["lvg_args"] = np.array(json.dumps(lvg_args))
    for name, kw in lvg_args.items():
        lv_ref = quiet(dsA.get_lvgs, **kw)
        assert len(lv_ref) == (kw.get("n") or n_hvg)
        out["A_lvg_" + name] = np.array([str(x) for x in lv_ref])
        col = ref_tab["fixed_var" if kw.get("use_corrected_var") else "variance"][valid]
        assert np.unique(col).shape[0] == col.shape[0], "two genes tie in the LVG sort"
        for what, tab in (("the reference's statistics", ref_tab), ("the restated statistics", mine_tab)):
            assert quiet(_qc.get_lvgs, tab, hvgs=out["A_hvg_explicit"], **kw) == list(out["A_lvg_" + name]), (name, what)
    # what nabo_amd._qc writes loads in the reference's Dataset
    fn_w = os.path.join(td, "written.h5")
    write_dataset(fn_w, cells, genes, XA)
    _qc._write_processed(fn_w, keep_cells_idx=out["A_keep_cells"], keep_genes_idx=out["A_keep_genes"], sf=out["A_sf"])
    _qc.dump_hvgs(fn_w, list(out["A_hvg_corrected"]))
    back = quiet(ds_mod.Dataset, fn_w, MITO_PATTERNS, RIBO_PATTERNS)
    for msg in ("INFO: Cached filtered cells loaded", "INFO: Cached filtered genes loaded", "INFO: Cached cell size factors loaded", "INFO: Loaded cached HVG names"):
        assert msg in quiet.last, msg
    assert np.array_equal(back.keepCellsIdx, dsA.keepCellsIdx) and back.keepCellsIdx.dtype == dsA.keepCellsIdx.dtype
    assert np.array_equal(back.keepGenesIdx, dsA.keepGenesIdx) and back.sf.dtype == np.float32 and np.array_equal(back.sf, out["A_sf"])
    assert back.hvgList == list(out["A_hvg_corrected"])

    out["tot_dev"], out["lowess_dev"], out["fixed_var_dev"] = np.float64(tot_dev), np.float64(lowess_dev), np.float64(fixed_var_dev)
    out["meta"] = np.array(json.dumps({"seed": SEED, "mito_patterns": MITO_PATTERNS, "ribo_patterns": RIBO_PATTERNS, "zero_gene": ZERO_GENE,
                                       "empty_cell": EMPTY_CELL}))
    fn = os.path.join(GOLD, "qc.npz")
    save_npz(fn, out)
    print("tot_dev %.3g, lowess_dev %.3g, fixed_var_dev %.3g" % (tot_dev, lowess_dev, fixed_var_dev))
    print("hvgs %s, lvgs %s" % ([len(out["A_hvg_" + k]) for k in ("corrected", "plain", "explicit")], [len(out["A_lvg_" + k]) for k in lvg_args]))
    print("wrote %s (%d bytes)" % (fn, os.path.getsize(fn)))


if __name__ == "__main__":
    sys.exit(main())
