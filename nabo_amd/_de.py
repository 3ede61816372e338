"""Differential expression by the Mann-Whitney U test, and cluster markers, on the GPU.

Array / HDF5 restatement of the reference's nabo/_marker.py: `run_de_test` (:12-114) and `find_cluster_markers`
(:117-169).  The per (gene, control group) work -- expressed fraction, log2 fold change, U, tie term, z, p -- comes from
`nabo_de_test` (include/nabo_de.h, nabo_amd/csrc/de_rank.hip); the carry-over of an empty group, Benjamini-Hochberg,
the ordering and the filter are host code.  The device step is kept apart from the host logic: the `_*_from_*` functions
take the per-pair arrays, and every function that needs them takes the step as an argument, so the logic is testable
without a GPU.
"""
import ctypes as C
from collections import Counter

import numpy as np

from . import _lib
from ._matrixio import DatasetFile as _DatasetFile, csc as _csc

SKIP_GENE, SKIP_PAIR, ASYMPTOTIC, EXACT, EMPTY = 0, 1, 2, 3, 4
COLUMNS = ["gene", "exp_frac", "test_group", "versus_group", "rbc", "log2_fc", "pval", "qval"]
_FIELDS = (("status", np.int32), ("nonzero_test", np.int64), ("n1", np.int64), ("n2", np.int64), ("u2", np.int64), ("tie", np.int64),
           ("log2_fc", np.float64), ("z", np.float64), ("pval", np.float64), ("rbc", np.float64))


# ---- arrays -------------------------------------------------------------------------------------------------------
def _device_de(n_genes, m1, m2, set_ptr, members, pair_test, pair_ctrl, exp_frac_thresh, log2_fc_thresh, mem_budget=0, device=0):
    """the device step: per-pair arrays of shape (n_genes, n_pairs), see de_test_csc.  m1, m2: _csc tuples, m2 or None"""
    n_pairs = len(pair_test)
    out = {k: np.zeros((n_genes, n_pairs), dtype=t) for k, t in _FIELDS}
    nul = (0, None, None, None, None)
    a = m1[:1] + tuple(x.ctypes.data for x in m1[1:])
    b = nul if m2 is None else m2[:1] + tuple(x.ctypes.data for x in m2[1:])
    _lib.check(_lib.lib().nabo_de_test(int(device), int(n_genes), *a, *b, int(set_ptr.shape[0] - 1), set_ptr.ctypes.data, members.ctypes.data,
                                       int(n_pairs), pair_test.ctypes.data, pair_ctrl.ctypes.data, float(exp_frac_thresh),
                                       float(log2_fc_thresh), int(mem_budget), *[out[k].ctypes.data for k, _ in _FIELDS]))
    return out


def last_device_ms():
    """({"expand": ms, "sort": ms, "rank": ms}, gene chunks) of this thread's last device step (nabo_de_last_device_ms)"""
    ms, chunks = (C.c_double * 3)(), C.c_int64()
    _lib.check(_lib.lib().nabo_de_last_device_ms(ms, C.byref(chunks)))
    return {"expand": ms[0], "sort": ms[1], "rank": ms[2]}, int(chunks.value)


def _sets(set_ptr, members):
    set_ptr, members = np.ascontiguousarray(set_ptr, dtype=np.int64), np.ascontiguousarray(members, dtype=np.int64)
    if set_ptr.ndim != 1 or members.ndim != 1 or set_ptr.shape[0] < 2:
        raise ValueError("ERROR: set_ptr needs n_sets + 1 >= 2 entries, members one entry per membership")
    if int(set_ptr[0]) != 0 or (np.diff(set_ptr) < 0).any() or int(set_ptr[-1]) != members.shape[0]:
        raise ValueError("ERROR: set_ptr must start at 0, be monotone and end at len(members)")
    return set_ptr, members


def de_test_csc(gene_ptr, cell, val, sf, set_ptr, members, matrix2=None, pair_test=None, pair_ctrl=None, exp_frac_thresh=0.25,
                log2_fc_thresh=1.0, mem_budget=0, device=0):
    """The Mann-Whitney test of every gene for every (test set, control set) pair (nabo_de_test, include/nabo_de.h).

    Expression as compressed sparse columns: gene g lists the cells cell[gene_ptr[g]:gene_ptr[g+1]] (strictly
    increasing) with values val[...]; a cell's value is float32(val * sf[cell]), 0 where not listed.  `matrix2`, a
    second (gene_ptr, cell, val, sf) with the same genes, is read by the control sets when given.  Set s is
    members[set_ptr[s]:set_ptr[s+1]] (repeats count).  Without pairs, set 0 is tested against sets 1, 2, ...; otherwise
    pair p tests set pair_test[p] against pair_ctrl[p].  Returns a dict of (n_genes, n_pairs) arrays: "status" (SKIP_GENE,
    SKIP_PAIR, ASYMPTOTIC, EXACT, EMPTY), "nonzero_test", "n1", "n2", "u2" (= 2 U1) and "tie" as int64, "log2_fc", "z",
    "pval", "rbc" as float64.  Scaled values must be finite and >= 0, a test set must not be empty: ValueError."""
    m1 = _csc((gene_ptr, cell, val, sf), "matrix 1")
    m2 = None if matrix2 is None else _csc(matrix2, "matrix 2")
    n_genes = m1[1].shape[0] - 1
    if m2 is not None and m2[1].shape[0] - 1 != n_genes:
        raise ValueError("ERROR: the two matrices hold %d and %d genes" % (n_genes, m2[1].shape[0] - 1))
    set_ptr, members = _sets(set_ptr, members)
    if (pair_test is None) != (pair_ctrl is None):
        raise ValueError("ERROR: give both pair_test and pair_ctrl, or neither")
    if pair_test is None:
        pair_test, pair_ctrl = np.zeros(set_ptr.shape[0] - 2, dtype=np.int32), np.arange(1, set_ptr.shape[0] - 1, dtype=np.int32)
    pair_test, pair_ctrl = np.ascontiguousarray(pair_test, dtype=np.int32), np.ascontiguousarray(pair_ctrl, dtype=np.int32)
    if pair_test.ndim != 1 or pair_test.shape != pair_ctrl.shape:
        raise ValueError("ERROR: pair_test and pair_ctrl must be 1-D and of one length")
    return _device_de(n_genes, m1, m2, set_ptr, members, pair_test, pair_ctrl, exp_frac_thresh, log2_fc_thresh, mem_budget, device)


# ---- the table ----------------------------------------------------------------------------------------------------
def _fdr_bh(pvals):
    """statsmodels' multipletests(pvals, method='fdr_bh')[1], operation by operation: p sorted ascending, divided by
    rank / n, running minimum from the largest down, capped at 1.  The running minimum gives equal p-values one
    q-value bit for bit, whatever order the sort left them in."""
    pvals = np.asarray(pvals, dtype=np.float64)
    n = pvals.shape[0]
    order = np.argsort(pvals, kind="stable")
    raw = pvals[order] / (np.arange(1, n + 1) / float(n))
    q = np.minimum.accumulate(raw[::-1])[::-1]
    q[q > 1] = 1
    out = np.empty_like(q)
    out[order] = q
    return out


def _rows_from_pairs(res, cols):
    """rows the reference's loop emits (nabo/_marker.py:69-102) for the pairs `cols` of one test set, in its order: gene
    by gene, group by group, every pair that was tested or whose control group is empty.  Returns (gene index, group
    index, exp_frac, rbc, log2_fc, pval).  An empty group takes rbc and pval from the last group of the same gene that
    reached the test, 0 and 1 if none did: what the reference's variables still hold when mannwhitneyu raises."""
    st = res["status"][:, cols]
    n_groups = st.shape[1]
    tested = (st == ASYMPTOTIC) | (st == EXACT)
    src = np.maximum.accumulate(np.where(tested, np.arange(n_groups)[None, :], -1), axis=1) if n_groups else st
    g, i = np.nonzero(tested | (st == EMPTY))
    from_ = src[g, i]
    rbc = np.where(from_ >= 0, res["rbc"][:, cols][g, np.maximum(from_, 0)], 0.0)
    pval = np.where(from_ >= 0, res["pval"][:, cols][g, np.maximum(from_, 0)], 1.0)
    exp_frac = res["nonzero_test"][:, cols][g, i] / res["n1"][:, cols][g, i]
    return g, i, exp_frac, rbc, res["log2_fc"][:, cols][g, i], pval


def _table_from_rows(genes, rows, test_label, group_labels, qval_thresh):
    """the reference's table (:104-114) as a dict of columns: q-values over all rows (NaN for a single row), rows ordered
    by (qval, emission order) -- the reference's sort is unstable among equal q-values -- and filtered qval < qval_thresh
    (which drops a NaN)."""
    g, i, exp_frac, rbc, log2_fc, pval = rows
    qval = _fdr_bh(pval) if g.shape[0] > 1 else np.full(g.shape[0], np.nan)
    order = np.argsort(qval, kind="stable")
    order = order[qval[order] < qval_thresh]
    return {"gene": [genes[k] for k in g[order].tolist()], "exp_frac": exp_frac[order].astype(np.float64),
            "test_group": [test_label] * order.shape[0], "versus_group": [group_labels[k] for k in i[order].tolist()],
            "rbc": rbc[order].astype(np.float64), "log2_fc": log2_fc[order].astype(np.float32), "pval": pval[order].astype(np.float64),
            "qval": qval[order].astype(np.float64)}


def _concat(tables):
    return {k: ([x for t in tables for x in t[k]] if k in ("gene", "test_group", "versus_group") else
                np.concatenate([t[k] for t in tables])) for k in COLUMNS}


def _as_frame(table):
    """a pandas DataFrame in the reference's column order when pandas can be imported, else the dict of columns"""
    try:
        import pandas as pd
    except ImportError:
        return table
    return pd.DataFrame({k: table[k] for k in COLUMNS}, columns=COLUMNS)


def _flatten(groups):
    ptr = np.zeros(len(groups) + 1, dtype=np.int64)
    np.cumsum([len(x) for x in groups], out=ptr[1:])
    return ptr, np.array([c for grp in groups for c in grp], dtype=np.int64)


def _de_from_csc(genes, m1, m2, test_idx, control_idx_groups, test_label, control_group_labels, exp_frac_thresh, log2_fc_thresh,
                 qval_thresh, step=_device_de):
    """run_de_test on arrays: genes (names, one per column), the matrices, the cell indices.  `step` is the device step
    (n_genes, m1, m2, set_ptr, members, pair_test, pair_ctrl, exp_frac_thresh, log2_fc_thresh) -> per-pair arrays"""
    if test_label is None:
        test_label = "Test group"
    if control_group_labels is None:
        control_group_labels = ["Ctrl group %d" % x for x in range(len(control_idx_groups))]
    if len(genes) and not len(test_idx):
        raise ZeroDivisionError("division by zero")            # the reference's expressed fraction of no cells (:74)
    n = len(control_idx_groups)
    if not len(genes) or not n:
        rows = tuple(np.zeros(0, dtype=t) for t in (np.int64, np.int64, np.float64, np.float64, np.float64, np.float64))
    else:
        set_ptr, members = _flatten([list(test_idx)] + [list(x) for x in control_idx_groups])
        res = step(len(genes), m1, m2, set_ptr, members, np.zeros(n, dtype=np.int32), np.arange(1, n + 1, dtype=np.int32),
                   exp_frac_thresh, log2_fc_thresh)
        rows = _rows_from_pairs(res, np.arange(n))
    return _table_from_rows(genes, rows, test_label, control_group_labels, qval_thresh)


def _markers_from_csc(clusters, genes, m1, de_frequency, exp_frac_thresh, log2_fc_thresh, qval_thresh, cell_idx, step=_device_de):
    """find_cluster_markers on arrays; cell_idx: {cell name: column}.  ONE device step for all clusters: the sets are the
    clusters in sorted order, the pairs every cluster against every other."""
    cluster_groups = {}
    for k, v in clusters.items():
        if v not in cluster_groups:
            cluster_groups[v] = []
        cluster_groups[v].append(k.rsplit("_", 1)[0])
    if de_frequency >= len(cluster_groups):
        de_frequency = len(cluster_groups) - 1
        print("WARNING: Value of 'de_frequency' reset to %d as number of clusters are %d" % (de_frequency, len(cluster_groups)))
    cluster_set = sorted(set(cluster_groups.keys()))
    if not cluster_set:
        raise ValueError("No objects to concatenate")            # the reference's pd.concat of no tables (:169)
    n = len(cluster_set)
    idx = [[cell_idx[x] for x in cluster_groups[c]] for c in cluster_set]
    res = None
    if n > 1 and len(genes):
        set_ptr, members = _flatten(idx)
        pt = np.repeat(np.arange(n, dtype=np.int32), n - 1)
        pc = np.array([j for i in range(n) for j in range(n) if j != i], dtype=np.int32)
        res = step(len(genes), m1, None, set_ptr, members, pt, pc, exp_frac_thresh, log2_fc_thresh)
    tables, de_genes = [], {}
    for t, c in enumerate(cluster_set):
        others = [x for x in cluster_set if x != c]
        if res is None:
            rows = tuple(np.zeros(0, dtype=d) for d in (np.int64, np.int64, np.float64, np.float64, np.float64, np.float64))
        else:
            rows = _rows_from_pairs(res, np.arange(t * (n - 1), (t + 1) * (n - 1)))
        tab = _table_from_rows(genes, rows, "Cluster %s" % str(c), ["Cluster %s" % str(x) for x in others], qval_thresh)
        tables.append(tab)
        de_genes[c] = [k for k, v in Counter(tab["gene"]).items() if v >= de_frequency]
    return _concat(tables), de_genes


# ---- the Nabo dataset file ----------------------------------------------------------------------------------------
def _valid_genes(d1, d2):
    """the genes the reference loops over (:57-66): the kept genes of dataset1 by name, repeats once, and with a second
    dataset only those it names too"""
    valid = {}
    other = None if d2 is None else {x: None for x in d2.genes}
    for i in d1.keep_genes_idx:
        gene = d1.genes[i]
        if other is None or gene in other:
            valid[gene] = None
    return list(valid)


def run_de_test(dataset1_h5, dataset2_h5, test_cells, control_cells, test_label=None, control_group_labels=None, exp_frac_thresh=0.25,
                log2_fc_thresh=1, qval_thresh=0.05, device=0):
    """nabo.run_de_test (nabo/_marker.py:12-114) on Nabo dataset files (`dataset1_h5`, and `dataset2_h5` or None, stand
    for the Dataset objects): differentially expressed genes of `test_cells` against every list of `control_cells`
    (cell names; the control lists name cells of dataset2 when it is given), by the Mann-Whitney U test on the MI355X.

    Returns the reference's table -- columns gene, exp_frac, test_group, versus_group, rbc, log2_fc, pval, qval -- as a
    pandas DataFrame when pandas can be imported, otherwise as a dict of columns (lists of str, numpy arrays).  The
    row set, exp_frac and rbc equal the reference's; quirks kept:
      * repeated cells count as often as they are listed, and a cell may be in the test list and in control lists;
      * only the min(n_test, n_group) largest values of a control group are used;
      * an empty control group still gives a row for every gene that passes exp_frac_thresh: log2_fc NaN, rbc and pval
        those of the last group of the same gene that reached the test (0 and 1 if none);
      * an empty test list raises ZeroDivisionError (if there is a gene to test); an unknown cell raises KeyError;
      * a single row has qval NaN and is dropped by the filter, whatever qval_thresh.
    Deviations: log2_fc comes from float64 means (the reference sums in float32) and is returned as float32 always (the
    reference's column turns float64 when an inf or NaN is among the rows); rows of equal qval keep the order of the
    reference's loop (its sort is unstable); scaled values must be finite and >= 0 and size factors float32
    (ValueError otherwise)."""
    d1 = _DatasetFile(dataset1_h5)
    d2 = None
    try:
        if dataset2_h5 is not None:
            d2 = _DatasetFile(dataset2_h5)
        test_idx = [d1.cell_idx[x] for x in test_cells]
        groups = [[(d1 if d2 is None else d2).cell_idx[x] for x in grp] for grp in control_cells]
        genes = _valid_genes(d1, d2)
        m1 = d1.csc(genes)
        m2 = None if d2 is None else d2.csc(genes)
    finally:
        d1.close()
        if d2 is not None:
            d2.close()

    def step(*a):
        return _device_de(*a, device=device)
    return _as_frame(_de_from_csc(genes, m1, m2, test_idx, groups, test_label, control_group_labels, exp_frac_thresh, log2_fc_thresh,
                                  qval_thresh, step))


def find_cluster_markers(clusters, dataset_h5, de_frequency, exp_frac_thresh=0.25, log2_fc_thresh=0.5, qval_thresh=0.05, device=0):
    """nabo.find_cluster_markers (nabo/_marker.py:117-169) on a Nabo dataset file: `clusters` maps node names
    (`<cell>_<sample>`) to clusters; every cluster, in sorted order, is tested against every other one.  Returns (table,
    {cluster: genes found against at least `de_frequency` other clusters}); the table is the concatenation of the
    per-cluster tables of run_de_test (a DataFrame with pandas, else a dict of columns).  `de_frequency` is clamped to the
    number of clusters minus 1, with the reference's warning.  All clusters go to the device in ONE call."""
    d = _DatasetFile(dataset_h5)
    try:
        genes = _valid_genes(d, None)
        m1 = d.csc(genes)
        cell_idx = d.cell_idx
    finally:
        d.close()

    def step(*a):
        return _device_de(*a, device=device)
    table, de_genes = _markers_from_csc(clusters, genes, m1, de_frequency, exp_frac_thresh, log2_fc_thresh, qval_thresh, cell_idx, step)
    return _as_frame(table), de_genes
