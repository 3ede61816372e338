"""Quality control of raw counts, size factors and the choice of highly variable genes: the step in front of the PCA.

Array / HDF5 restatement of the reference's nabo/_dataset.py: `filter_data` (:342-425 over :208-287), `set_sf`
(:548-592), `correct_var` (:639-683), `find_hvgs` (:685-755), `dump_hvgs` (:757-770) and `get_lvgs` (:772-812).  The
per-cell work -- a cell's total, the number of genes it lists, the cumulative expression of gene classes -- is ONE pass
of `nabo_cell_qc` (include/nabo_qc.h, nabo_amd/csrc/cell_qc.hip) over the cells; the per-gene statistics are
`nabo_gene_stats` (_pca.py).  Thresholds, percentages and size factors are the reference's own float32 expressions on
the host, so its comparisons come out as they do there.  As in _pca.py the device step is kept apart from the host
logic: the `_*_from_*` functions take the step as an argument, so the logic is testable without a GPU.
"""
import ctypes as C
import re

import numpy as np

from . import _lib, _pca
from ._matrixio import DatasetFile as _DatasetFile, csr as _csr, index_list as _index_list, ptr as _ptr

LDS_TABLE_GENES = 65536             # QC_LDS_TABLE_GENES of cell_qc.hip: up to here the class table is staged in LDS
MITO_PATTERNS = ("^MT-",)           # Dataset.__init__'s defaults (:128-132)
RIBO_PATTERNS = ("^RPS", "^RPL", "^MRPS", "^MRPL")
STAT_COLUMNS = ("valid_gene", "m", "nzm", "variance", "ncells")


# ---- arrays -------------------------------------------------------------------------------------------------------
def _device_qc(cell_ptr, gene, val, gene_class, n_classes, rows=None, mem_budget=0, device=0):
    """the device step: (n_entries int64 [n_rows], sums float64 [n_rows, 1 + n_classes]).  Arrays as _csr returns them;
    gene_class uint8 [n_raw_genes]; rows int64 or None"""
    n_cells, n_classes = cell_ptr.shape[0] - 1, int(n_classes)
    n_rows = n_cells if rows is None else rows.shape[0]
    n_ent = np.zeros(n_rows, dtype=np.int64)
    sums = np.zeros((n_rows, 1 + max(0, min(n_classes, 8))), dtype=np.float64)
    _lib.check(_lib.lib().nabo_cell_qc(int(device), n_cells, gene_class.shape[0], cell_ptr.ctypes.data, gene.ctypes.data, val.ctypes.data,
                                       n_classes, gene_class.ctypes.data if gene_class.shape[0] else np.zeros(1, np.uint8).ctypes.data,
                                       n_rows, _ptr(rows), int(mem_budget), n_ent.ctypes.data if n_rows else np.zeros(1, np.int64).ctypes.data,
                                       sums.ctypes.data if n_rows else np.zeros(1).ctypes.data))
    return n_ent, sums


def last_device_ms():
    """({"upload": ms, "kernel": ms, "download": ms}, chunks) of this thread's last nabo_cell_qc (nabo_qc_last_device_ms)"""
    ms, chunks = (C.c_double * 3)(), C.c_int64()
    _lib.check(_lib.lib().nabo_qc_last_device_ms(ms, C.byref(chunks)))
    return {"upload": ms[0], "kernel": ms[1], "download": ms[2]}, int(chunks.value)


def cell_qc_csr(cell_ptr, gene, val, gene_class=None, n_classes=0, rows=None, mem_budget=0, device=0):
    """Per-cell sums in one pass on the MI355X (nabo_cell_qc, include/nabo_qc.h).

    Expression as compressed sparse rows: cell i lists the raw genes gene[cell_ptr[i]:cell_ptr[i+1]] (strictly
    increasing) with the float32 values val[...], finite and >= 0.  gene_class[n_raw_genes], uint8: bit c < n_classes
    (at most 8 classes) marks the genes of class c; None stands for no class, and then the number of raw genes is taken
    as 1 + the largest listed gene.  `rows`: the cells in output order (None: all).  Returns (n_entries int64
    [n_rows], sums float64 [n_rows, 1 + n_classes]): column 0 the cell's total, column 1 + c the total over the genes
    of class c, float64 sums in the header's fixed order -- the same bits on every run and for every chunking.  Bad input
    raises ValueError before any device is touched."""
    cell_ptr, gene, val = _csr((cell_ptr, gene, val))
    if gene_class is None:
        if int(n_classes) != 0:
            raise ValueError("ERROR: n_classes=%d without gene_class" % int(n_classes))
        gene_class = np.zeros(int(gene.max()) + 1 if gene.size else 0, dtype=np.uint8)
    gene_class = np.ascontiguousarray(gene_class, dtype=np.uint8)
    if gene_class.ndim != 1:
        raise ValueError("ERROR: gene_class must be 1-D, one byte per raw gene")
    return _device_qc(cell_ptr, gene, val, gene_class, n_classes, _index_list(rows, "rows"), mem_budget, device)


# ---- the host logic: cells and genes to keep, size factors -----------------------------------------------------------
def genes_by_pattern(genes, patterns):
    """Dataset.get_genes_by_pattern (:274-287): the names `re.match` finds for any of the patterns, a sorted set"""
    out = []
    for sp in patterns:
        out.extend([x for x in genes if re.match(sp, x) is not None])
    return sorted(set(out))


def _class_columns(raw_genes, names):
    """the columns get_cum_exp (:208-232) adds up for `names`: every name is looked up in UPPER case, and one whose
    upper-case form the file does not hold is skipped silently.  Deviation: two names that resolve to one column (the
    reference would count it twice) raise ValueError."""
    idx = {x: n for n, x in enumerate(raw_genes)}
    cols = []
    for x in names:
        c = idx.get(x.upper())
        if c is not None:
            if c in cols:
                raise ValueError("ERROR: gene %s is counted twice: two matched names have the upper-case form %s" % (raw_genes[c], x.upper()))
            cols.append(c)
    return np.array(cols, dtype=np.int64)


def _filter_from_sums(n_entries, tot, cum_mito, cum_ribo, gene_abundance, keep_cells_idx, keep_genes_idx, mito_idx, ribo_idx,
                      min_exp=1000, max_exp=np.inf, min_ngenes=100, max_ngenes=np.inf, min_mito=-1, max_mito=101, min_ribo=-1, max_ribo=101,
                      min_gene_abundance=10, rm_mito=True, rm_ribo=True):
    """the decisions of filter_data (:369-405), literally, from the per-cell sums of ALL raw cells: totals and
    cumulative sums as float32, `100 * cum / tot` in float32 (a total of 0 gives NaN, which no comparison removes), the
    eight comparisons, `gene_abundance < min_gene_abundance` on the number of stored entries per gene, the mito / ribo
    genes by their own index, the intersection with the incoming keep lists, sorted.  Returns (keep_cells int64,
    keep_genes int64, counts): counts holds the eight numbers of the report, (low, high) for UMI, genes, mito, ribo."""
    f32 = np.float32
    tot = np.asarray(tot, dtype=np.float64).astype(f32)
    ngenes = np.asarray(n_entries).astype(f32)
    with np.errstate(divide="ignore", invalid="ignore"):
        percent_mito = f32(100) * np.asarray(cum_mito, dtype=np.float64).astype(f32) / tot
        percent_ribo = f32(100) * np.asarray(cum_ribo, dtype=np.float64).astype(f32) / tot
    assert percent_mito.dtype == f32 and percent_ribo.dtype == f32
    with np.errstate(invalid="ignore", over="ignore"):
        lists = [np.where(tot < f32(min_exp))[0], np.where(tot > f32(max_exp))[0],
                 np.where(ngenes < f32(min_ngenes))[0], np.where(ngenes > f32(max_ngenes))[0],
                 np.where(percent_mito < f32(min_mito))[0], np.where(percent_mito > f32(max_mito))[0],
                 np.where(percent_ribo < f32(min_ribo))[0], np.where(percent_ribo > f32(max_ribo))[0]]
    remove_cells = set(int(i) for a in lists for i in a)
    keep_cells = np.array(sorted(set(int(i) for i in keep_cells_idx).difference(remove_cells)), dtype=np.int64)
    if min_gene_abundance < 0:
        print("'min_gene_abundance' should be greater than or equal to 0")
        print("Resetting 'min_gene_abundance' to 0", flush=True)
        min_gene_abundance = 0
    remove_genes = set(int(i) for i in np.where(np.asarray(gene_abundance).astype(f32) < f32(min_gene_abundance))[0])
    if rm_mito:
        remove_genes.update(int(i) for i in mito_idx)
    if rm_ribo:
        remove_genes.update(int(i) for i in ribo_idx)
    keep_genes = np.array(sorted(set(int(i) for i in keep_genes_idx).difference(remove_genes)), dtype=np.int64)
    return keep_cells, keep_genes, [int(a.shape[0]) for a in lists]


def _report(counts):
    """the four lines filter_data prints with verbose=True (:407-414)"""
    return ["%s: Low: %d High: %d" % (what, counts[2 * i], counts[2 * i + 1])
            for i, what in enumerate(("UMI filtered  ", "Gene filtered ", "Mito filtered ", "Ribo filtered "))]


def _sf_from_sums(kept_sum, size_scale):
    """the size factors of set_sf (:574-584) from the cells' sums: float32(float64(size_scale) / float64(float32(sum))),
    a sum of 0 replaced by 1 -- the reference divides a Python float by a float32 scalar, which is a float64 division,
    and stores the quotient in its float32 vector"""
    s = np.asarray(kept_sum, dtype=np.float64).astype(np.float32)
    s[s == 0] = np.float32(1)
    return (np.float64(size_scale) / s.astype(np.float64)).astype(np.float32)


def _size_scale(size_scale):
    try:
        return float(size_scale)
    except TypeError:
        raise TypeError("ERROR: size_scale parameter should have a float value. E.x. not 1 but 1.0")


def _classes(raw_genes, keep_genes_idx, mito_patterns, ribo_patterns):
    """(gene_class uint8 with bit 0 mito, bit 1 ribo, bit 2 kept; mito_idx, ribo_idx: the matched names' own indices)"""
    mito = genes_by_pattern(raw_genes, MITO_PATTERNS if mito_patterns is None else mito_patterns)
    ribo = genes_by_pattern(raw_genes, RIBO_PATTERNS if ribo_patterns is None else ribo_patterns)
    gene_idx = {x: n for n, x in enumerate(raw_genes)}
    cls = np.zeros(len(raw_genes), dtype=np.uint8)
    cls[_class_columns(raw_genes, mito)] |= 1
    cls[_class_columns(raw_genes, ribo)] |= 2
    if keep_genes_idx is not None:
        cls[np.asarray(keep_genes_idx, dtype=np.int64)] |= 4
    return cls, [gene_idx[x] for x in mito], [gene_idx[x] for x in ribo]


def _filter_from_csr(raw_genes, m, gene_abundance, keep_cells_idx, keep_genes_idx, mito_patterns=None, ribo_patterns=None, step=_device_qc,
                     **thresholds):
    """filter_data on arrays: raw_genes names the genes of the (cell_ptr, gene, val) tuple `m` over ALL raw cells.
    Returns (keep_cells, keep_genes, counts) as _filter_from_sums does."""
    cls, mito_idx, ribo_idx = _classes(raw_genes, None, mito_patterns, ribo_patterns)
    n_ent, sums = step(*_csr(m), cls, 2)
    return _filter_from_sums(n_ent, sums[:, 0], sums[:, 1], sums[:, 2], gene_abundance, keep_cells_idx, keep_genes_idx, mito_idx, ribo_idx,
                             **thresholds)


def _sf_from_csr(cells, n_raw_genes, m, keep_genes_idx, sf_now, sf=None, size_scale=1000.0, all_genes=False, step=_device_qc):
    """set_sf on arrays: the float32 size factors of all raw cells.  With a `sf` dict (cell name -> size factor) the
    named cells of the vector in use, `sf_now`, are replaced by size_scale / sf[name] (:568-570) and no sum is taken."""
    size_scale = _size_scale(size_scale)
    if sf is not None:
        cell_idx = {x: n for n, x in enumerate(cells)}
        out = np.array(sf_now, dtype=np.float32)
        for i in sf:
            out[cell_idx[i]] = size_scale / sf[i]
        return out
    cls = np.zeros(n_raw_genes, dtype=np.uint8)
    if all_genes:
        _, sums = step(*_csr(m), cls, 0)
        return _sf_from_sums(sums[:, 0], size_scale)
    cls[np.asarray(keep_genes_idx, dtype=np.int64)] = 1
    _, sums = step(*_csr(m), cls, 1)
    return _sf_from_sums(sums[:, 1], size_scale)


def _qc_and_sf_from_csr(raw_genes, m, gene_abundance, keep_cells_idx, keep_genes_idx, mito_patterns=None, ribo_patterns=None, size_scale=1000.0,
                        all_genes=False, step=_device_qc, **thresholds):
    """filter_data followed by set_sf with ONE device pass and three class bits (mito, ribo, kept).  Which genes are
    kept depends on the genes' abundances, the patterns and the incoming list alone -- on nothing the device computes
    -- so the kept bit is known before the pass, also with all_genes=False.  Returns (keep_cells, keep_genes, counts,
    sf)."""
    size_scale = _size_scale(size_scale)
    cls, mito_idx, ribo_idx = _classes(raw_genes, None, mito_patterns, ribo_patterns)
    n_cells = len(m[0]) - 1
    _, keep_genes, _ = _filter_from_sums(np.zeros(n_cells), np.zeros(n_cells), np.zeros(n_cells), np.zeros(n_cells), gene_abundance, [],
                                         keep_genes_idx, mito_idx, ribo_idx, **thresholds)
    cls[keep_genes] |= 4
    n_ent, sums = step(*_csr(m), cls, 3)
    kw = dict(thresholds)
    if kw.get("min_gene_abundance", 0) < 0:
        kw["min_gene_abundance"] = 0                        # (the two lines were printed above)
    keep_cells, keep_genes, counts = _filter_from_sums(n_ent, sums[:, 0], sums[:, 1], sums[:, 2], gene_abundance, keep_cells_idx, keep_genes_idx,
                                                       mito_idx, ribo_idx, **kw)
    return keep_cells, keep_genes, counts, _sf_from_sums(sums[:, 0] if all_genes else sums[:, 3], size_scale)


# ---- the statistics table, the variance correction, HVGs and LVGs -------------------------------------------------
def _table(stats):
    """(gene names, dict of the columns as numpy arrays) of either form of the statistics table"""
    if isinstance(stats, dict):
        names, cols = [str(x) for x in stats["genes"]], {k: np.asarray(v) for k, v in stats.items() if k != "genes"}
    else:
        names, cols = [str(x) for x in stats.index], {k: stats[k].values for k in stats.columns}
    cols["valid_gene"] = np.asarray(cols["valid_gene"]).astype(bool)
    for k in cols:
        if k != "valid_gene":
            cols[k] = np.asarray(cols[k], dtype=np.float64)
    return names, cols


def _as_table(names, cols):
    """a pandas DataFrame indexed by gene when pandas can be imported, else a dict with "genes" and the columns"""
    try:
        import pandas as pd
    except ImportError:
        return dict({"genes": list(names)}, **cols)
    return pd.DataFrame(cols, index=list(names))


def _stats_table(names, st):
    """the reference's geneStats (:631-636) from the device's statistics: what an invalid gene lacks is the column's
    minimum over the valid genes, its ncells 0"""
    valid = np.asarray(st["valid"]).astype(bool)
    cols = {"valid_gene": valid}
    for k in ("m", "nzm", "variance"):
        a = np.array(st[k], dtype=np.float64)
        a[~valid] = a[valid].min() if valid.any() else np.nan
        cols[k] = a
    cols["ncells"] = np.where(valid, st["ncells"], 0).astype(np.float64)
    return _as_table(names, cols)


def lowess(y, x, frac, it):
    """statsmodels' `lowess(y, x, frac, it, delta=0, return_sorted=False)` (its _smoothers_lowess, third-party and
    public) restated in numpy float64: k = int(frac n + 1e-10) nearest neighbours of every x, tricube weights times the
    robustness weights, a local linear fit, then bisquare robustness weights from the residuals over 6 times their
    median, `it` times.  Iterating stops early once the robustness weights repeat bit for bit: every further
    iteration would give the same fit."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    if not 0 <= frac <= 1:
        raise ValueError("Lowess `frac` must be in the range [0,1]!")
    order = np.argsort(x)
    x, y = x[order], y[order]
    n = x.shape[0]
    k = int(frac * n + 1e-10)
    resid_w = np.ones(n)
    fit = np.zeros(n)
    for _ in range(int(it) + 1):
        fit = np.zeros(n)
        left, right = 0, k
        for i in range(n):
            xv = x[i]
            while right < n and xv > (x[left] + x[right]) / 2.0:
                left, right = left + 1, right + 1
            radius = max(xv - x[left], x[right - 1] - xv)
            xs = x[left:right]
            with np.errstate(divide="ignore", invalid="ignore"):
                d = np.abs(xs - xv) / radius
            t = 1.0 - d * d * d
            w = t * t * t * resid_w[left:right]
            sw = w.sum()
            if not sw > 0.0 or np.count_nonzero(w) == 1:
                fit[i] = y[i]
                continue
            w = w / sw
            swx = 0.0
            for j in range(w.shape[0]):
                swx += w[j] * xs[j]
            dev = xs - swx
            sq = 0.0
            for j in range(w.shape[0]):
                sq += w[j] * dev[j] * dev[j]
            if sq < 1e-12:
                sq = 1e-12
            p = w * (1.0 + (xv - swx) * dev / sq)
            acc = 0.0
            ys = y[left:right]
            for j in range(w.shape[0]):
                acc += p[j] * ys[j]
            fit[i] = acc
        r = np.abs(y - fit)
        med = np.median(r)
        if med == 0:
            r = (r > 0).astype(np.float64)
        else:
            r = r / (6.0 * med)
        r[r >= 1.0] = 1.0
        new_w = (1.0 - r * r) ** 2
        if np.array_equal(new_w, resid_w):
            break
        resid_w = new_w
    out = np.empty(n)
    out[order] = fit
    return out


def correct_var(stats, n_bins=100, lowess_frac=0.4):
    """Dataset.correct_var (:639-683) on the statistics table: removes the mean-variance trend.  The valid genes' log
    means are cut into n_bins bins (numpy's histogram edges, the last one + 0.1); per non-empty bin the gene of smallest
    log variance (the first in table order on a tie) gives one (variance, mean) point; a LOWESS curve through the points
    (`lowess`, it=100) is the bins' correction, and fixed_var = e ** (log variance - correction of the gene's bin); an
    invalid gene gets the column's minimum.  Returns (the table with `fixed_var` added, geneBinsMin,
    varCorrectionFactor)."""
    names, cols = _table(stats)
    valid = cols["valid_gene"]
    with np.errstate(divide="ignore", invalid="ignore"):
        lm, lv = np.log(cols["m"][valid]), np.log(cols["variance"][valid])
    n_bins = int(n_bins)
    edges = np.histogram(lm, bins=n_bins)[1]
    edges[-1] += 0.1
    bin_genes, bin_vals = [], []
    for i in range(n_bins):
        idx = np.nonzero((lm >= edges[i]) & (lm < edges[i + 1]))[0]
        if idx.shape[0] > 0:
            g = idx[np.argmin(lv[idx])]
            bin_genes.append(idx)
            bin_vals.append([lv[g], lm[g]])
    bin_vals = np.array(bin_vals).T
    cor = lowess(bin_vals[0], bin_vals[1], lowess_frac, 100)
    fixed_valid = np.full(lm.shape[0], np.nan)
    for bcf, idx in zip(cor, bin_genes):
        fixed_valid[idx] = np.e ** (lv[idx] - bcf)
    fixed = np.full(len(names), np.nan)
    fixed[valid] = fixed_valid
    fixed[np.isnan(fixed)] = np.nanmin(fixed) if (~np.isnan(fixed)).any() else np.nan
    cols["fixed_var"] = fixed
    return _as_table(names, cols), bin_vals[1], cor


def find_hvgs(stats, var_min_thresh=None, nzm_min_thresh=None, var_max_thresh=np.inf, nzm_max_thresh=np.inf, min_cells=0,
              use_corrected_var=False, dataset_h5=None, update_cache=False):
    """Dataset.find_hvgs (:685-755) on the statistics table, without the plot: the names of the highly variable genes
    in table order.  Quirks kept: thresholds are in log scale only with use_corrected_var; the defaults are
    np.percentile(nzm, 5) and np.percentile(variance or fixed_var, 95) over the valid genes; without correction the
    variance threshold is a percentile of `variance` but is compared against variance / m.  With update_cache=True the
    list goes to `processed_data/hvg_list` of `dataset_h5` (dump_hvgs)."""
    names, cols = _table(stats)
    if use_corrected_var is True and "fixed_var" not in cols:
        raise ValueError('ERROR: "use_corrected_var" parameter is set to True. Either  run "correct_var" method first or set '
                         '"use_corrected_var" to False')
    valid = cols["valid_gene"]
    gs = {k: v[valid] for k, v in cols.items() if k != "valid_gene"}
    if use_corrected_var:
        with np.errstate(divide="ignore", invalid="ignore"):
            gs = {k: (v if k == "ncells" else np.log(v)) for k, v in gs.items()}
    if nzm_min_thresh is None:
        nzm_min_thresh = np.percentile(gs["nzm"], 5)
    if var_min_thresh is None:
        var_min_thresh = np.percentile(gs["fixed_var" if use_corrected_var else "variance"], 95)
    with np.errstate(divide="ignore", invalid="ignore"):
        v = gs["fixed_var"] if use_corrected_var else gs["variance"] / gs["m"]
        cand = (v > var_min_thresh) & (gs["nzm"] > nzm_min_thresh) & (v < var_max_thresh) & (gs["nzm"] < nzm_max_thresh) & (gs["ncells"] > min_cells)
    hvgs = [names[i] for i in np.nonzero(valid)[0][cand]]
    if update_cache:
        if dataset_h5 is None:
            raise ValueError("ERROR: update_cache=True needs dataset_h5, the file to write the list to")
        dump_hvgs(dataset_h5, hvgs)
    print("%d highly variable genes found" % len(hvgs), flush=True)
    return hvgs


def get_lvgs(stats, nzm_cutoff=None, log_nzm_cutoff=None, n=None, use_corrected_var=False, hvgs=None):
    """Dataset.get_lvgs (:772-812) on the statistics table: the n valid genes of least (corrected) variance among those
    with a non-zero mean above the cutoff; n defaults to the number of `hvgs`.  Genes of equal variance come in table
    order (the reference's sort is an unstable quicksort)."""
    names, cols = _table(stats)
    if use_corrected_var is True and "fixed_var" not in cols:
        raise ValueError('ERROR: "use_fixed_var" parameter is set to True. Either  run "correct_var" method first or set '
                         '"use_fixed_var" to False')
    use_var = "fixed_var" if use_corrected_var else "variance"
    if nzm_cutoff is None and log_nzm_cutoff is None:
        raise ValueError("ERROR: Please provide a value for either of the two parameters: `nzm_cutoff` and `log_nzm_cutoff`")
    if nzm_cutoff is not None and log_nzm_cutoff is not None:
        raise ValueError("ERROR: Please provide a value for only ONE the two parameters: `nzm_cutoff` and `log_nzm_cutoff`")
    cutoff = nzm_cutoff if nzm_cutoff is not None else np.e ** log_nzm_cutoff
    if n is None:
        n = len(hvgs)
    sel = np.nonzero(cols["valid_gene"] & (cols["nzm"] > cutoff))[0]
    if sel.shape[0] < n:
        print('WARNING: Number of LVGs is lower than "n"/HVGs. Try reducing "nzm_cutoff"')
    order = np.argsort(cols[use_var][sel], kind="stable")
    return [names[i] for i in sel[order][:n]]


# ---- the Nabo dataset file ----------------------------------------------------------------------------------------
def _read_all(dataset_h5):
    """(cells, genes, keep_cells_idx, keep_genes_idx, sf, the CSR of ALL raw cells, the stored entries per gene)"""
    d = _DatasetFile(dataset_h5)
    try:
        ptr, gene, val, sf = d.csr(range(len(d.cells)))
        gd = d.h5["gene_data"]
        abundance = np.array([gd[g].shape[0] for g in d.genes], dtype=np.int64)     # get_gene_abundance (:260-272)
        return d.cells, d.genes, d.keep_cells_idx, d.keep_genes_idx, sf, (ptr, gene, val), abundance
    finally:
        d.close()


def _write_processed(dataset_h5, **datasets):
    """replaces datasets of `processed_data`, as the reference does (:416-424, :586-591, :764-770)"""
    from ._mapping import _h5py
    try:
        h5 = _h5py().File(dataset_h5, mode="a")
    except Exception:
        raise IOError("ERROR: Could not open file %s" % dataset_h5)
    try:
        grp = h5["processed_data"] if "processed_data" in h5 else h5.create_group("processed_data")
        for k, v in datasets.items():
            if k in grp:
                del grp[k]
            grp.create_dataset(k, data=v)
        h5.flush()
    finally:
        h5.close()


def _thresholds(min_exp, max_exp, min_ngenes, max_ngenes, min_mito, max_mito, min_ribo, max_ribo, min_gene_abundance, rm_mito, rm_ribo):
    return dict(min_exp=min_exp, max_exp=max_exp, min_ngenes=min_ngenes, max_ngenes=max_ngenes, min_mito=min_mito, max_mito=max_mito,
                min_ribo=min_ribo, max_ribo=max_ribo, min_gene_abundance=min_gene_abundance, rm_mito=rm_mito, rm_ribo=rm_ribo)


def filter_data(dataset_h5, min_exp=1000, max_exp=np.inf, min_ngenes=100, max_ngenes=np.inf, min_mito=-1, max_mito=101, min_ribo=-1,
                max_ribo=101, min_gene_abundance=10, rm_mito=True, rm_ribo=True, verbose=True, mito_patterns=None, ribo_patterns=None,
                mem_budget=0, device=0):
    """Dataset.filter_data (:342-425) on a Nabo dataset file, with the two pattern lists of Dataset.__init__: removes
    cells by total, number of genes and the percentages of mitochondrial and ribosomal expression, genes by the number
    of cells that list them and by pattern, from the keep lists the file holds (all, when it holds none), prints the
    reference's report and writes `processed_data/keep_cells_idx` and `keep_genes_idx`.  The per-cell sums are one pass
    of the MI355X over the cells, in float64 (the reference sums in float32: equal for integer counts with totals below
    2^24).  Returns (keep_cells_idx, keep_genes_idx)."""
    cells, genes, kc, kg, _, m, abundance = _read_all(dataset_h5)

    def step(*a):
        return _device_qc(*a, mem_budget=mem_budget, device=device)
    keep_cells, keep_genes, counts = _filter_from_csr(genes, m, abundance, kc, kg, mito_patterns, ribo_patterns, step,
                                                      **_thresholds(min_exp, max_exp, min_ngenes, max_ngenes, min_mito, max_mito, min_ribo,
                                                                    max_ribo, min_gene_abundance, rm_mito, rm_ribo))
    if verbose:
        for ln in _report(counts):
            print(ln, flush=True)
    _write_processed(dataset_h5, keep_cells_idx=keep_cells, keep_genes_idx=keep_genes)
    return keep_cells, keep_genes


def set_sf(dataset_h5, sf=None, size_scale=1000.0, all_genes=False, mem_budget=0, device=0):
    """Dataset.set_sf (:548-592) on a Nabo dataset file: the size factor of every raw cell, size_scale over the cell's
    sum over the kept genes (all_genes=True: over all genes; a sum of 0 counts as 1), float32, written to
    `processed_data/sf`.  A `sf` dict (cell name -> size factor) instead replaces the named cells' entries of the stored
    vector by size_scale / sf[name].  size_scale=None raises the reference's TypeError.  Returns the vector."""
    size_scale = _size_scale(size_scale)
    cells, genes, _, kg, sf_now, m, _ = _read_all(dataset_h5)

    def step(*a):
        return _device_qc(*a, mem_budget=mem_budget, device=device)
    out = _sf_from_csr(cells, len(genes), m, kg, sf_now, sf, size_scale, all_genes, step)
    _write_processed(dataset_h5, sf=out)
    return out


def qc_and_sf(dataset_h5, min_exp=1000, max_exp=np.inf, min_ngenes=100, max_ngenes=np.inf, min_mito=-1, max_mito=101, min_ribo=-1,
              max_ribo=101, min_gene_abundance=10, rm_mito=True, rm_ribo=True, verbose=True, mito_patterns=None, ribo_patterns=None,
              size_scale=1000.0, all_genes=False, mem_budget=0, device=0):
    """filter_data followed by set_sf: the file is read once and the cells are passed over ONCE, with three class bits
    (mito, ribo, kept) -- the kept genes follow from the genes' abundances, the patterns and the stored list, so they are
    known before the pass, with all_genes=False too.  Writes what the two functions write and returns (keep_cells_idx,
    keep_genes_idx, sf)."""
    cells, genes, kc, kg, _, m, abundance = _read_all(dataset_h5)

    def step(*a):
        return _device_qc(*a, mem_budget=mem_budget, device=device)
    keep_cells, keep_genes, counts, sf = _qc_and_sf_from_csr(genes, m, abundance, kc, kg, mito_patterns, ribo_patterns, size_scale, all_genes, step,
                                                             **_thresholds(min_exp, max_exp, min_ngenes, max_ngenes, min_mito, max_mito, min_ribo,
                                                                           max_ribo, min_gene_abundance, rm_mito, rm_ribo))
    if verbose:
        for ln in _report(counts):
            print(ln, flush=True)
    _write_processed(dataset_h5, keep_cells_idx=keep_cells, keep_genes_idx=keep_genes, sf=sf)
    return keep_cells, keep_genes, sf


def dump_hvgs(dataset_h5, hvgs):
    """Dataset.dump_hvgs (:757-770): writes the names to `processed_data/hvg_list`, replacing the list"""
    _write_processed(dataset_h5, hvg_list=[x.encode("ascii") for x in hvgs])


def gene_stats(dataset_h5, device=0):
    """Dataset.set_gene_stats (:594-637) on a Nabo dataset file: the statistics table of ALL genes in file order, with
    the columns valid_gene, m, nzm, variance (population) and ncells of the normalised values over the kept cells, from
    nabo_gene_stats on the MI355X.  A gene that is not kept or has no positive value is not valid; its m, nzm and
    variance are the columns' minima over the valid genes, its ncells 0.  A pandas DataFrame indexed by gene when pandas
    can be imported, otherwise a dict with "genes" and the columns.  Deviation: float64 sums over the float32 values."""
    d = _DatasetFile(dataset_h5)
    try:
        raw_genes, keep_genes_idx, keep_cells = d.genes, d.keep_genes_idx, d.keep_cells_idx
        kept = sorted(set(keep_genes_idx))                       # only these columns are read; the others stay empty
        mk = d.csc([raw_genes[i] for i in kept], upper=False)
        ptr = np.zeros(len(raw_genes) + 1, dtype=np.int64)
        ptr[np.array(kept, dtype=np.int64) + 1] = np.diff(mk[1])
        m = (mk[0], np.cumsum(ptr), mk[2], mk[3], mk[4])
    finally:
        d.close()
    keep = np.zeros(len(raw_genes), dtype=np.uint8)
    keep[np.asarray(keep_genes_idx, dtype=np.int64)] = 1
    st = _pca._device_stats(m, np.ascontiguousarray(keep_cells, dtype=np.int64), keep, device=device)
    return _stats_table(raw_genes, st)
