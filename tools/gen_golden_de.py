#!/opt/conda/bin/python3.9
"""Golden vectors for the differential-expression functions of the reference (nabo/_marker.py): run_de_test (:12-114)
and find_cluster_markers (:117-169).

TEST INFRASTRUCTURE ONLY, run where the reference is mounted, with an interpreter that has h5py, pandas, scipy >= 1.7
and statsmodels:

    /opt/conda/bin/python3.9 tools/gen_golden_de.py

The reference's nabo/_dataset.py and nabo/_marker.py are loaded BY FILE PATH under a stub `nabo` package (numba replaced
by an identity `jit`, as oracle/gen_golden.py does).  Seeded synthetic datasets are written as Nabo-format HDF5 files
into a temporary directory, the reference runs on them, and only DATA goes to tests/golden/de.npz: the sparse matrices,
size factors, names, the cell lists of every call and the reference's tables, unfiltered (qval_thresh = 2).

Two measured values are stored with them, against the tests' own restatement (tests/_de_ref.py):
  log2fc_dev  the largest |reference log2_fc (float32 sums) - restated log2_fc (float64 sums)| over all rows with a
              finite log2_fc;
  p_dev       the largest relative difference between the reference's p and the restated p (math.erfc; the exact
              distribution in integers) over all rows with p > 0.
The script asserts that no pair of any case has a log2_fc within 5 * log2fc_dev of the case's threshold (the tests allow
4), so that the skip decisions, and with them the row sets, must match exactly.  A grid value that fails is moved.
"""
import contextlib
import importlib.util
import io
import json
import math
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
import _de_ref as dref  # noqa: E402

# (exp_frac_thresh, log2_fc_thresh): the reference's defaults of run_de_test and of find_cluster_markers, everything
# tested (an all-zero test sample included), and two stricter ones
DE_GRID = [(0.25, 1.0), (0.25, 0.5), (0.0, -4.0), (0.5, 0.26), (0.1, 2.0)]


def load_reference():
    nb = types.ModuleType("numba")
    nb.jit = lambda *a, **k: (a[0] if len(a) == 1 and callable(a[0]) and not k else (lambda f: f))
    sys.modules["numba"] = nb
    pkg = types.ModuleType("nabo")
    pkg.__path__ = []
    sys.modules["nabo"] = pkg
    mods = {}
    for name in ("_dataset", "_marker"):
        spec = importlib.util.spec_from_file_location("nabo." + name, os.path.join(REF, "nabo", name + ".py"))
        m = importlib.util.module_from_spec(spec)
        sys.modules["nabo." + name] = m
        spec.loader.exec_module(m)
        mods[name] = m
    return mods["_dataset"], mods["_marker"]


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fn(*a, **k)


def synth(rng, n_cells, genes, n_blocks, density, continuous=()):
    """a sparse cells x genes matrix of counts with block structure: gene j is expressed mostly in block j % n_blocks.
    Genes named in `continuous` hold distinct positive floats in every cell (no zeros, no ties)."""
    block = np.arange(n_cells) * n_blocks // n_cells
    cols = []
    for j, g in enumerate(genes):
        if g in continuous:
            cols.append((np.arange(n_cells), (rng.permutation(n_cells) + 1 + rng.random(n_cells) * 0.5).astype(np.float32)
                         * np.where(block == j % n_blocks, 3.0, 1.0).astype(np.float32)))
            continue
        p = np.where(block == j % n_blocks, min(1.0, density * (1 + j % 6)), density * (0.5 if j % 3 else 1.0))
        idx = np.nonzero(rng.random(n_cells) < p)[0]
        val = rng.poisson(np.where(block[idx] == j % n_blocks, 1.5 * 2 ** (j % 5 * 0.5), 1.5)).astype(np.float32) + (1 if j % 4 else 0)
        cols.append((idx, val))                                  # (j % 4 == 0: a few stored zeros)
    return cols


def write_dataset(fn, cells, genes, cols, sf, keep_genes_idx):
    import h5py
    with h5py.File(fn, "w") as h5:
        g = h5.create_group("names")
        g.create_dataset("cells", data=np.array([x.encode() for x in cells]))
        g.create_dataset("genes", data=np.array([x.encode() for x in genes]))
        gd = h5.create_group("gene_data")
        for name, (idx, val) in zip(genes, cols):
            d = np.zeros(len(idx), dtype=[("idx", np.uint32), ("val", np.float32)])
            d["idx"], d["val"] = idx, val
            gd.create_dataset(name, data=d)
        if sf is not None:
            p = h5.create_group("processed_data")
            p.create_dataset("sf", data=sf)
            if keep_genes_idx is not None:
                p.create_dataset("keep_genes_idx", data=np.array(keep_genes_idx))


def store(out, prefix, cells, genes, cols, sf, keep_genes_idx):
    out[prefix + "_cells"], out[prefix + "_genes"] = np.array(cells), np.array(genes)
    out[prefix + "_gene_ptr"] = np.concatenate([[0], np.cumsum([len(i) for i, _ in cols])]).astype(np.int64)
    out[prefix + "_cell"] = np.concatenate([i for i, _ in cols]).astype(np.int32)
    out[prefix + "_val"] = np.concatenate([v for _, v in cols]).astype(np.float32)
    out[prefix + "_sf"] = np.ones(len(cells), np.float32) if sf is None else sf
    out[prefix + "_keep"] = np.arange(len(genes)) if keep_genes_idx is None else np.array(keep_genes_idx)


def table_json(df):
    return {c: [x if isinstance(x, str) else float(x) for x in df[c].tolist()] for c in
            ("gene", "exp_frac", "test_group", "versus_group", "rbc", "log2_fc", "pval", "qval")}


class Measure:
    """the reference's rows against the restatement: deviations, and the distance of every log2_fc from the threshold"""

    def __init__(self):
        self.log2fc_dev, self.p_dev, self.margins = 0.0, 0.0, []

    def add(self, name, table, res, genes, labels, log2_fc_thresh):
        st = res["status"]
        for g, i in zip(*np.nonzero((st != dref.SKIP_GENE) & (st != dref.EMPTY))):
            if math.isfinite(res["log2_fc"][g, i]):
                self.margins.append((abs(res["log2_fc"][g, i] - log2_fc_thresh), name, genes[g], labels[i]))
        where = {(genes[g], labels[i]): (g, i) for g, i in zip(*np.nonzero((st == dref.ASYMPTOTIC) | (st == dref.EXACT)))}
        seen = 0
        for gene, grp, lfc, p, rbc in zip(table["gene"], table["versus_group"], table["log2_fc"], table["pval"], table["rbc"]):
            if (gene, grp) not in where:
                continue                                        # an empty group's row: carried values
            g, i = where[(gene, grp)]
            seen += 1
            assert rbc == res["rbc"][g, i], (name, gene, grp, rbc, res["rbc"][g, i])
            if math.isfinite(lfc):
                self.log2fc_dev = max(self.log2fc_dev, abs(lfc - res["log2_fc"][g, i]))
            else:
                assert lfc == res["log2_fc"][g, i]
            if p > 0:
                self.p_dev = max(self.p_dev, abs(p - res["pval"][g, i]) / p)
            else:
                assert res["pval"][g, i] == 0
        return seen


def restate(d, prefix, prefix2, genes, test_idx, groups_idx, ef, lfc):
    m1 = dref.csc_of(d, prefix)
    m2 = None if prefix2 is None else dref.csc_of(d, prefix2)
    for m, pre in ((m1, prefix), (m2, prefix2)):
        if m is not None:                                       # the columns of `genes`, in that order
            names = [str(x) for x in d[pre + "_genes"]]
            sel = [names.index(g) for g in genes]
            ptr = m[1]
            cell = np.concatenate([m[2][ptr[j]:ptr[j + 1]] for j in sel] + [np.zeros(0, np.int32)])
            val = np.concatenate([m[3][ptr[j]:ptr[j + 1]] for j in sel] + [np.zeros(0, np.float32)])
            gp = np.concatenate([[0], np.cumsum([ptr[j + 1] - ptr[j] for j in sel])]).astype(np.int64)
            if pre == prefix:
                m1 = (m[0], gp, cell, val, m[4])
            else:
                m2 = (m[0], gp, cell, val, m[4])
    sets = [list(test_idx)] + [list(x) for x in groups_idx]
    set_ptr = np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.int64)
    members = np.array([c for s in sets for c in s], dtype=np.int64)
    n = len(groups_idx)
    return dref.de_step(len(genes), m1, m2, set_ptr, members, np.zeros(n, np.int32), np.arange(1, n + 1, dtype=np.int32), ef, lfc)


def valid_genes(d, prefix, prefix2):
    names = [str(x) for x in d[prefix + "_genes"]]
    other = None if prefix2 is None else set(str(x) for x in d[prefix2 + "_genes"])
    out = {}
    for i in d[prefix + "_keep"].tolist():
        if other is None or names[i] in other:
            out[names[i]] = None
    return list(out)


def main():
    ds_mod, mk = load_reference()
    rng = np.random.default_rng(20240611)
    out, cases, meas = {}, [], Measure()
    td = tempfile.mkdtemp()

    # ---- dataset 1 (240 cells x 60 genes, 52 kept), dataset 2 (150 cells, 48 of the genes and 6 others, other order)
    cells1 = ["c%d" % i for i in range(240)]
    genes1 = ["G%d" % i for i in range(60)]
    cols1 = synth(rng, 240, genes1, 4, 0.12, continuous=("G7", "G33"))
    sf1 = (0.5 + rng.random(240) * 1.5).astype(np.float32)
    keep1 = [i for i in range(60) if i % 8 != 5]
    cells2 = ["d%d" % i for i in range(150)]
    genes2 = [genes1[i] for i in rng.permutation(60)[:48]] + ["H%d" % i for i in range(6)]
    cols2 = synth(rng, 150, genes2, 3, 0.10, continuous=("G7",))
    sf2 = (0.5 + rng.random(150) * 1.5).astype(np.float32)
    fn1, fn2 = os.path.join(td, "d1.h5"), os.path.join(td, "d2.h5")
    write_dataset(fn1, cells1, genes1, cols1, sf1, keep1)
    write_dataset(fn2, cells2, genes2, cols2, sf2, None)
    store(out, "d1", cells1, genes1, cols1, sf1, keep1)
    store(out, "d2", cells2, genes2, cols2, sf2, None)
    ds1, ds2 = quiet(ds_mod.Dataset, fn1), quiet(ds_mod.Dataset, fn2)

    def run(name, prefix, prefix2, d_a, d_b, test, groups, ef, lfc, labels=None, test_label=None):
        try:
            df = quiet(mk.run_de_test, d_a, d_b, test, groups, test_label, labels, exp_frac_thresh=ef, log2_fc_thresh=lfc, qval_thresh=2)
            res, table = "ok", table_json(df)
        except Exception as e:  # noqa: BLE001 -- the exception type is the recorded result
            res, table = type(e).__name__, None
        case = {"name": name, "d1": prefix, "d2": prefix2, "test_cells": test, "control_cells": groups, "test_label": test_label,
                "labels": labels, "exp_frac_thresh": ef, "log2_fc_thresh": lfc, "result": res, "table": table}
        cases.append(case)
        if table is not None:
            ci_a = {str(x): i for i, x in enumerate(out[prefix + "_cells"])}
            ci_b = ci_a if prefix2 is None else {str(x): i for i, x in enumerate(out[prefix2 + "_cells"])}
            genes = valid_genes(out, prefix, prefix2)
            r = restate(out, prefix, prefix2, genes, [ci_a[x] for x in test], [[ci_b[x] for x in grp] for grp in groups], ef, lfc)
            lab = labels or ["Ctrl group %d" % i for i in range(len(groups))]
            seen = meas.add(name, table, r, genes, lab, lfc)
            case["unfiltered_rows"] = int(((r["status"] >= dref.ASYMPTOTIC)).sum())
            print("  %-28s %4d rows (%d matched), %d exact" % (name, len(table["gene"]), seen, int((r["status"] == dref.EXACT).sum())))
        else:
            print("  %-28s %s" % (name, res))
        return case

    test1 = cells1[:60]
    groups1 = [cells1[60:120], cells1[120:200], cells1[200:240]]                # the middle one larger than the test list
    test12 = cells1[10:70]
    groups2 = [cells2[:50], cells2[50:100], cells2[100:150]]
    for ef, lfc in DE_GRID:
        run("grid_%g_%g" % (ef, lfc), "d1", None, ds1, None, test1, groups1, ef, lfc)
        run("grid2_%g_%g" % (ef, lfc), "d1", "d2", ds1, ds2, test12, groups2, ef, lfc, labels=["A", "B", "C"], test_label="T")

    # ---- find_cluster_markers: 4 clusters over dataset 1's cells, node names carry the sample suffix
    clusters = {"%s_S" % c: int(i * 4 // 240) + 1 for i, c in enumerate(cells1)}
    for key, freq, ef, lfc in (("markers", 2, 0.25, 0.5), ("markers_clamped", 9, 0.1, 1.0)):
        df, de_genes = quiet(mk.find_cluster_markers, clusters, ds1, freq, exp_frac_thresh=ef, log2_fc_thresh=lfc, qval_thresh=0.05)
        out[key] = np.array(json.dumps({"clusters": clusters, "de_frequency": freq, "exp_frac_thresh": ef, "log2_fc_thresh": lfc,
                                        "qval_thresh": 0.05, "table": table_json(df), "de_genes": {str(k): v for k, v in de_genes.items()}}))
        print("  %-28s %4d rows, %s genes" % (key, df.shape[0], {k: len(v) for k, v in de_genes.items()}))
        # the margins of every per-cluster call
        genes = valid_genes(out, "d1", None)
        ci = {c: i for i, c in enumerate(cells1)}
        byc = {}
        for k, v in clusters.items():
            byc.setdefault(v, []).append(ci[k.rsplit("_", 1)[0]])
        for c in sorted(byc):
            others = [x for x in sorted(byc) if x != c]
            r = restate(out, "d1", None, genes, byc[c], [byc[x] for x in others], ef, lfc)
            meas.add("%s_%s" % (key, c), {k: [] for k in ("gene", "versus_group", "log2_fc", "pval", "rbc")}, r, genes,
                     ["Cluster %s" % x for x in others], lfc)

    # ---- the quirk dataset: 40 cells x 12 genes, no size factors, every gene kept
    cellsq = ["q%d" % i for i in range(40)]
    genesq = ["Q%d" % i for i in range(12)]
    colsq = synth(rng, 40, genesq, 2, 0.3, continuous=("Q1", "Q4", "Q9"))
    colsq[2] = (np.arange(0, 6), np.array([3, 1, 4, 1, 5, 9], np.float32))      # Q2: in the first six cells only
    colsq[3] = (np.zeros(0, np.int64), np.zeros(0, np.float32))                 # Q3: no nonzero at all
    fnq = os.path.join(td, "q.h5")
    write_dataset(fnq, cellsq, genesq, colsq, None, None)
    store(out, "q", cellsq, genesq, colsq, None, None)
    dsq = quiet(ds_mod.Dataset, fnq)
    tq = cellsq[:6]
    gq = [[], cellsq[6:11], [], cellsq[6:18], cellsq[3:10], [cellsq[12]] * 3 + cellsq[12:15], cellsq[20:28], []]
    run("quirk_groups", "q", None, dsq, None, tq, gq, 0.25, -20.0)              # empty first / middle / last, truncation, overlap, repeats, n <= 8
    run("quirk_all", "q", None, dsq, None, tq, gq, 0.0, -20.0)                  # the all-zero gene is tested too
    run("quirk_repeated_test", "q", None, dsq, None, tq + tq[:3], [cellsq[6:20], tq], 0.25, -20.0)
    run("quirk_large_vs_small", "q", None, dsq, None, cellsq[:14], [cellsq[20:25], cellsq[14:40]], 0.9, -20.0)
    run("quirk_ctrl_mean_zero", "q", None, dsq, None, tq, [cellsq[30:36]], 0.25, 1.0)
    run("quirk_empty_test", "q", None, dsq, None, [], [cellsq[6:11]], 0.25, 1.0)
    run("quirk_only_empty", "q", None, dsq, None, tq, [[]], 0.25, 1.0)
    run("quirk_unknown_cell", "q", None, dsq, None, tq + ["nobody"], [cellsq[6:11]], 0.25, 1.0)
    # a single row: the threshold between the two largest finite log2_fc of one group
    c = run("probe", "q", None, dsq, None, tq, [cellsq[5:15]], 0.25, -20.0)
    cases.pop()
    top = sorted((x for x in c["table"]["log2_fc"] if math.isfinite(x)), reverse=True)
    assert not any(math.isinf(x) for x in c["table"]["log2_fc"]) and top[0] - top[1] > 1e-3
    c = run("quirk_single_row", "q", None, dsq, None, tq, [cellsq[5:15]], 0.25, (top[0] + top[1]) / 2)
    assert c["unfiltered_rows"] == 1 and c["table"]["gene"] == []                # its qval is NaN: the filter drops it

    want = {"quirk_groups": "ok", "quirk_empty_test": "ZeroDivisionError", "quirk_unknown_cell": "KeyError", "quirk_only_empty": "ok"}
    for c in cases:
        if c["name"] in want:
            assert c["result"] == want[c["name"]], (c["name"], c["result"])
    for c in cases:
        if c["name"].startswith("quirk_groups"):
            t = c["table"]
            assert any(math.isnan(x) for x in t["log2_fc"]) and "Ctrl group 0" in t["versus_group"] and "Ctrl group 2" in t["versus_group"]
            first = [(r, p) for g, r, p in zip(t["versus_group"], t["rbc"], t["pval"]) if g == "Ctrl group 0"]
            assert all(r == 0 and p == 1 for r, p in first)      # nothing to carry in front of the first group
    # the deviations, and the margins against them
    assert 0 < meas.log2fc_dev < 1e-5 and meas.p_dev < 1e-12, (meas.log2fc_dev, meas.p_dev)
    near = sorted(m for m in meas.margins if m[0] <= 5 * meas.log2fc_dev)
    assert not near, near[:5]
    out["cases"] = np.array(json.dumps(cases))
    out["log2fc_dev"], out["p_dev"] = np.float64(meas.log2fc_dev), np.float64(meas.p_dev)
    fn = os.path.join(GOLD, "de.npz")
    np.savez_compressed(fn, **out)
    print("log2fc_dev %.3g, p_dev %.3g, closest margin %.3g" % (meas.log2fc_dev, meas.p_dev, min(m[0] for m in meas.margins)))
    print("wrote %s (%d bytes; classify.npz is %d)" % (fn, os.path.getsize(fn), os.path.getsize(os.path.join(GOLD, "classify.npz"))))


if __name__ == "__main__":
    sys.exit(main())
