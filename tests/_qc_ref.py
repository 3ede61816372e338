"""Plain restatements of include/nabo_qc.h and of the host logic of filter_data and set_sf (nabo/_dataset.py:342-425,
:548-592) for the tests and for tools/gen_golden_qc.py, independent of nabo_amd/_qc.py.  numpy's float64 `+` is a
single IEEE operation; the sums are taken in the header's order: 16 partial sums, entry e to partial sum e mod 16 in
ascending e, then the butterfly over 8, 4, 2, 1."""
import math
import re

import numpy as np

GROUP = 16
_J = np.arange(GROUP)


def ordered_sum(x):
    """the header's sum of the float64 values x (in stored order)"""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    pad = np.zeros(-(-max(n, 1) // GROUP) * GROUP, dtype=np.float64)
    pad[:n] = x
    s = np.zeros(GROUP, dtype=np.float64)
    for row in pad.reshape(-1, GROUP):
        s = s + row
    for d in (8, 4, 2, 1):
        s = s + s[_J ^ d]
    return s[0]


def cell_qc(cell_ptr, gene, val, gene_class=None, n_classes=0, rows=None, exact=False):
    """(n_entries int64 [n_rows], sums float64 [n_rows, 1 + n_classes]) by the header's definition; exact=True: exactly
    rounded sums (math.fsum) instead of the header's order"""
    cell_ptr, gene = np.asarray(cell_ptr, dtype=np.int64), np.asarray(gene, dtype=np.int64)
    val = np.asarray(val, dtype=np.float32)
    rows = np.arange(cell_ptr.shape[0] - 1) if rows is None else np.asarray(rows, dtype=np.int64)
    total = (lambda x: math.fsum(x.tolist())) if exact else ordered_sum
    n_ent = np.zeros(rows.shape[0], dtype=np.int64)
    sums = np.zeros((rows.shape[0], 1 + n_classes), dtype=np.float64)
    for r, c in enumerate(rows.tolist()):
        a, b = int(cell_ptr[c]), int(cell_ptr[c + 1])
        x = val[a:b].astype(np.float64)
        n_ent[r] = b - a
        sums[r, 0] = total(x)
        for k in range(n_classes):
            member = ((np.asarray(gene_class)[gene[a:b]].astype(np.int64) >> k) & 1).astype(bool)
            sums[r, 1 + k] = total(np.where(member, x, 0.0))      # an entry outside the class adds 0.0
    return n_ent, sums


def cell_qc_many(cell_ptr, gene, val, gene_class=None, n_classes=0):
    """cell_qc over all cells, for tests with very many short cells: a cell of at most 16 entries has one entry per
    partial sum, so its sum is the butterfly over its values padded to 16 with +0.0 (0.0 + x first, as ordered_sum adds
    the row to its zeros), taken for all such cells at once; a longer cell goes through ordered_sum"""
    cell_ptr, gene = np.asarray(cell_ptr, dtype=np.int64), np.asarray(gene, dtype=np.int64)
    val = np.asarray(val, dtype=np.float32)
    n_ent = np.diff(cell_ptr)
    sums = np.zeros((n_ent.shape[0], 1 + n_classes), dtype=np.float64)
    short = np.nonzero(n_ent <= GROUP)[0]
    at = cell_ptr[short][:, None] + _J[None, :]
    inside = _J[None, :] < n_ent[short][:, None]
    at = at[inside]                                              # the short cells' entries, cell by cell
    cls = np.asarray(gene_class, dtype=np.int64)[gene] if n_classes else None
    for k in range(1 + n_classes):
        x = val.astype(np.float64)
        if k > 0:
            x = np.where(((cls >> (k - 1)) & 1).astype(bool), x, 0.0)     # an entry outside the class adds 0.0
        pad = np.zeros((short.shape[0], GROUP), dtype=np.float64)
        pad[inside] = x[at]
        s = np.zeros_like(pad) + pad
        for d in (8, 4, 2, 1):
            s = s + s[:, _J ^ d]
        sums[short, k] = s[:, 0]
        for c in np.nonzero(n_ent > GROUP)[0].tolist():
            sums[c, k] = ordered_sum(x[cell_ptr[c]:cell_ptr[c + 1]])
    return n_ent.astype(np.int64), sums


def step(cell_ptr, gene, val, gene_class, n_classes):
    """cell_qc with the signature of nabo_amd._qc's device step"""
    return cell_qc(cell_ptr, gene, val, gene_class, n_classes)


# ---- filter_data and set_sf, from the cells' sums -------------------------------------------------------------------
def pattern_genes(genes, patterns):
    return sorted(set(x for sp in patterns for x in genes if re.match(sp, x) is not None))


def class_bits(genes, mito_patterns, ribo_patterns, keep_genes=None):
    """bit 0: the columns get_cum_exp adds up for the mito names (looked up in upper case, skipped when absent); bit 1:
    ribo; bit 2: the kept genes"""
    genes = [str(g) for g in genes]
    where = {g: i for i, g in enumerate(genes)}
    cls = np.zeros(len(genes), dtype=np.uint8)
    for bit, pats in ((1, mito_patterns), (2, ribo_patterns)):
        for name in pattern_genes(genes, pats):
            if name.upper() in where:
                cls[where[name.upper()]] |= bit
    if keep_genes is not None:
        cls[np.asarray(keep_genes, dtype=np.int64)] |= 4
    return cls


def filter_ref(genes, n_entries, sums, abundance, keep_cells, keep_genes, mito_patterns, ribo_patterns, thr):
    """(keep_cells, keep_genes, the report's eight counts); sums[:, 0:3] = total, mito, ribo; thr: filter_data's keywords"""
    genes = [str(g) for g in genes]
    f = np.float32
    tot, ng = sums[:, 0].astype(f), np.asarray(n_entries).astype(f)
    with np.errstate(all="ignore"):
        pm, pr = f(100) * sums[:, 1].astype(f) / tot, f(100) * sums[:, 2].astype(f) / tot
        crit = [tot < f(thr["min_exp"]), tot > f(thr["max_exp"]), ng < f(thr["min_ngenes"]), ng > f(thr["max_ngenes"]),
                pm < f(thr["min_mito"]), pm > f(thr["max_mito"]), pr < f(thr["min_ribo"]), pr > f(thr["max_ribo"])]
    gone = np.zeros(tot.shape[0], dtype=bool)
    for c in crit:
        gone |= c
    kc = np.array([i for i in sorted(set(int(x) for x in keep_cells)) if not gone[i]], dtype=np.int64)
    drop = np.asarray(abundance) < max(0, thr["min_gene_abundance"])
    where = {g: i for i, g in enumerate(genes)}
    if thr.get("rm_mito", True):
        drop[[where[g] for g in pattern_genes(genes, mito_patterns)]] = True
    if thr.get("rm_ribo", True):
        drop[[where[g] for g in pattern_genes(genes, ribo_patterns)]] = True
    kg = np.array([i for i in sorted(set(int(x) for x in keep_genes)) if not drop[i]], dtype=np.int64)
    return kc, kg, [int(c.sum()) for c in crit]


def sf_ref(sum_per_cell, size_scale):
    """float32(float64(size_scale) / float64(float32(sum))), a sum of 0 counted as 1"""
    s = np.asarray(sum_per_cell, dtype=np.float64).astype(np.float32)
    out = np.empty(s.shape[0], dtype=np.float32)
    for i, v in enumerate(s.tolist()):
        out[i] = float(size_scale) / (v if v != 0 else 1.0)
    return out


# ---- the golden file (tests/golden/qc.npz, tools/gen_golden_qc.py) --------------------------------------------------
def csr_of(d, s):
    return d[s + "_cell_ptr"], d[s + "_gene"], d[s + "_val"]


def thresholds_of(d, s):
    import json
    return json.loads(str(d[s + "_thresholds"]))


def patterns_of(d):
    import json
    m = json.loads(str(d["meta"]))
    return m["mito_patterns"], m["ribo_patterns"]


def stats_of(d, s, fixed=None):
    """the reference's geneStats of sample s as the dict form of the statistics table"""
    t = {"genes": [str(g) for g in d["genes"]], "valid_gene": d[s + "_stats_valid"].astype(bool)}
    for k in ("m", "nzm", "variance", "ncells"):
        t[k] = d[s + "_stats_" + k].astype(np.float64)
    if fixed is not None:
        t["fixed_var"] = d[s + "_fixed_var_%d" % fixed]
    return t
