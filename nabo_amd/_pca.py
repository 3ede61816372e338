"""Projection of sparse cells into a fitted PCA space, the per-gene statistics behind the scaling parameters, and the fit
of the PCA itself, on the GPU.

Array / HDF5 restatement of the reference's nabo/_dataset.py: `set_gene_stats` (:594-637), `get_scaling_params`
(:814-844), `get_scaled_values` (:846-915) and `transform_pca` (:985-1033).  The per-cell and per-gene work comes from
`nabo_pca_project` and `nabo_gene_stats` (include/nabo_pca.h, nabo_amd/csrc/pca_project.hip); which genes are valid,
their order, the missing-gene rules and the HDF5 layouts are host code.  `fit_ipca` (:917-983) becomes an exact fit: the
mean and the covariance of the scaled cells come from `nabo_pca_cov` (include/nabo_pca_fit.h, nabo_amd/csrc/pca_fit.hip),
the eigen-decomposition of that G x G matrix is numpy's on the host.  As in _de.py the device step is kept apart from
the host logic: the `_*_from_*` functions take the step as an argument, so the logic is testable without a GPU.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._matrixio import DatasetFile as _DatasetFile, csc as _csc, csr as _csr, index_list as _index_list, int32 as _int32, ptr as _ptr

_STAT_FIELDS = (("ncells", np.int64), ("valid", np.uint8), ("m", np.float64), ("nzm", np.float64), ("variance", np.float64))


# ---- arrays -------------------------------------------------------------------------------------------------------
def _device_project(m, gene_pos, mu, sigma, mean, components, rows, mem_budget=0, device=0):
    """the device step of the projection: Z[n_rows, C].  m: a _csr tuple; the tables checked by _tables; rows int64 or None"""
    n_rows = m[0] if rows is None else rows.shape[0]
    Z = np.zeros((n_rows, components.shape[0]), dtype=np.float64)
    _lib.check(_lib.lib().nabo_pca_project(int(device), m[0], gene_pos.shape[0], m[1].ctypes.data, m[2].ctypes.data, m[3].ctypes.data,
                                           m[4].ctypes.data, gene_pos.ctypes.data, mu.shape[0], mu.ctypes.data, sigma.ctypes.data,
                                           mean.ctypes.data, components.shape[0], components.ctypes.data, n_rows,
                                           _ptr(rows), int(mem_budget), Z.ctypes.data if Z.size else np.zeros(1).ctypes.data))
    return Z


def _device_stats(m, keep_cells, keep_genes, device=0):
    """the device step of the statistics: a dict of per-gene arrays.  m: a _csc tuple; keep_cells int64 or None;
    keep_genes uint8 or None"""
    n_genes = m[1].shape[0] - 1
    out = {k: np.zeros(n_genes, dtype=t) for k, t in _STAT_FIELDS}
    _lib.check(_lib.lib().nabo_gene_stats(int(device), n_genes, m[0], m[1].ctypes.data, m[2].ctypes.data, m[3].ctypes.data, m[4].ctypes.data,
                                          0 if keep_cells is None else keep_cells.shape[0], _ptr(keep_cells),
                                          None if keep_genes is None else keep_genes.ctypes.data, *[out[k].ctypes.data for k, _ in _STAT_FIELDS]))
    return out


def last_device_ms():
    """({"upload": ms, "kernel": ms, "download": ms}, chunks) of this thread's last device step (nabo_pca_last_device_ms)"""
    ms, chunks = (C.c_double * 3)(), C.c_int64()
    _lib.check(_lib.lib().nabo_pca_last_device_ms(ms, C.byref(chunks)))
    return {"upload": ms[0], "kernel": ms[1], "download": ms[2]}, int(chunks.value)


def _device_cov(m, gene_pos, mu, sigma, rows, mem_budget=0, device=0):
    """the device step of the fit: (mean[G], cov[G, G]).  m: a _csr tuple; the tables checked by _fit_tables; rows int64 or None"""
    G = mu.shape[0]
    mean, cov = np.zeros(G, dtype=np.float64), np.zeros((G, G), dtype=np.float64)
    _lib.check(_lib.lib().nabo_pca_cov(int(device), m[0], gene_pos.shape[0], m[1].ctypes.data, m[2].ctypes.data, m[3].ctypes.data, m[4].ctypes.data,
                                       gene_pos.ctypes.data, G, mu.ctypes.data, sigma.ctypes.data, m[0] if rows is None else rows.shape[0],
                                       _ptr(rows), int(mem_budget), mean.ctypes.data, cov.ctypes.data))
    return mean, cov


def last_cov_phase_ms():
    """{"column_sums": ms, "densify": ms, "product": ms} of this thread's last nabo_pca_cov (nabo_pca_cov_last_phase_ms)"""
    ms = (C.c_double * 3)()
    _lib.check(_lib.lib().nabo_pca_cov_last_phase_ms(ms))
    return {"column_sums": ms[0], "densify": ms[1], "product": ms[2]}


def cov_resident_bytes(n_sel_genes):
    """what nabo_pca_cov keeps resident beside the chunks of rows, and the bytes of one row without its entries
    (include/nabo_pca_fit.h): a budget of resident + k * (row + 8 * entries per row) holds k rows per chunk"""
    nt = (int(n_sel_genes) + 127) // 128
    t = nt * (nt + 1) // 2
    s = min(16, max(1, -(-1024 // t)))
    return t * 131072 * (1 + s) + nt * 128 * 2048, 12 + 8 * nt * 128


def _fit_tables(gene_pos, mu, sigma):
    gene_pos = _int32(gene_pos, "gene_pos")
    mu, sigma = (np.ascontiguousarray(x, dtype=np.float64) for x in (mu, sigma))
    if gene_pos.ndim != 1 or mu.ndim != 1 or sigma.ndim != 1 or mu.shape[0] < 1 or sigma.shape[0] != mu.shape[0]:
        raise ValueError("ERROR: gene_pos, mu and sigma must be 1-D, mu and sigma over the same n_genes >= 1 genes")
    return gene_pos, mu, sigma


def _tables(gene_pos, mu, sigma, mean, components):
    gene_pos = _int32(gene_pos, "gene_pos")
    mu, sigma, mean = (np.ascontiguousarray(x, dtype=np.float64) for x in (mu, sigma, mean))
    components = np.ascontiguousarray(components, dtype=np.float64)
    if gene_pos.ndim != 1 or mu.ndim != 1 or sigma.ndim != 1 or mean.ndim != 1 or components.ndim != 2:
        raise ValueError("ERROR: gene_pos, mu, sigma and mean must be 1-D, components 2-D [n_comps, n_genes]")
    G = mu.shape[0]
    if sigma.shape[0] != G or mean.shape[0] != G or components.shape[1] != G or components.shape[0] < 1 or G < 1:
        raise ValueError("ERROR: mu holds %d genes, sigma %d, mean %d, components has shape %s: need [n_comps >= 1, %d]"
                         % (G, sigma.shape[0], mean.shape[0], components.shape, G))
    return gene_pos, mu, sigma, mean, components


def pca_project_csr(cell_ptr, gene, val, sf, gene_pos, mu, sigma, mean, components, rows=None, mem_budget=0, device=0):
    """Projects sparse cells onto PCA components (nabo_pca_project, include/nabo_pca.h): what the reference's
    `transformer.transform([a])` gives for the scaled vector `a` of get_scaled_values, without the dense vector.

    Expression as compressed sparse rows: cell i lists the raw genes gene[cell_ptr[i]:cell_ptr[i+1]] (strictly
    increasing) with values val[...]; the value is float32(val * sf[i]).  gene_pos[raw gene] is the gene's position
    among the G selected genes or -1; mu, sigma (> 0), mean are [G], components [C, G] as sklearn stores them.  `rows`:
    the cells to project in output order (None: all).  Returns Z[len(rows), C] float64, bit for bit the sequential
    definition in the header.  Bad input raises ValueError before any device is touched."""
    m = _csr((cell_ptr, gene, val, sf))
    t = _tables(gene_pos, mu, sigma, mean, components)
    return _device_project(m, *t, _index_list(rows, "rows"), mem_budget, device)


def gene_stats_csc(gene_ptr, cell, val, sf, keep_cells=None, keep_genes=None, device=0):
    """Per-gene statistics of the normalised values float32(val * sf[cell]) over the kept cells (nabo_gene_stats): a dict
    of arrays "ncells" (int64), "valid" (uint8), "m", "nzm", "variance" (float64; the population variance), 0 for a
    gene that is not kept or has no positive value.  Expression as compressed sparse columns, as for de_test_csc."""
    m = _csc((gene_ptr, cell, val, sf), "the matrix")
    n_genes = m[1].shape[0] - 1
    if keep_genes is not None:
        keep_genes = np.ascontiguousarray(np.asarray(keep_genes) != 0, dtype=np.uint8)
        if keep_genes.shape != (n_genes,):
            raise ValueError("ERROR: keep_genes must hold one entry per gene (%d)" % n_genes)
    return _device_stats(m, _index_list(keep_cells, "keep_cells"), keep_genes, device)


def pca_cov_csr(cell_ptr, gene, val, sf, gene_pos, mu, sigma, rows=None, mem_budget=0, device=0):
    """Mean and sample covariance (divisor n - 1) of the scaled cells (nabo_pca_cov, include/nabo_pca_fit.h): of the
    vectors ((float32(val * sf[cell]) - mu) / sigma over the G selected genes, 0 where a cell lists nothing) the
    reference's get_scaled_values yields, without the dense matrix.  Arguments as for pca_project_csr; at least 2 rows.
    Returns (mean[G], cov[G, G]) float64; two passes, deterministic, cov symmetric bit for bit.  Bad input raises
    ValueError before any device is touched."""
    m = _csr((cell_ptr, gene, val, sf))
    return _device_cov(m, *_fit_tables(gene_pos, mu, sigma), _index_list(rows, "rows"), mem_budget, device)


# ---- the host logic -----------------------------------------------------------------------------------------------
def _scaling_from_csc(raw_genes, keep_genes_idx, m, keep_cells, genes=None, only_valid=True, step=_device_stats):
    """get_scaling_params on arrays: raw_genes names the columns of the _csc tuple `m`.  Returns (names, mu, sigma).
    geneStats is keyed by gene name: a name the file holds twice keeps its first place and its last column."""
    keep = np.zeros(len(raw_genes), dtype=np.uint8)
    keep[np.asarray(keep_genes_idx, dtype=np.int64)] = 1
    st = step(m, None if keep_cells is None else np.ascontiguousarray(keep_cells, dtype=np.int64), keep)
    col = {}
    for i, g in enumerate(raw_genes):
        col[g] = i
    valid = st["valid"].astype(bool)
    with np.errstate(invalid="ignore"):
        mu, sigma = st["m"].astype(np.float64), np.sqrt(st["variance"].astype(np.float64))
    cols = np.array(list(col.values()), dtype=np.int64)
    named_valid = cols[valid[cols]]
    # the reference fills what an invalid gene lacks with the column's minimum (:632-634)
    mu[~valid] = mu[named_valid].min() if named_valid.size else np.nan
    sigma[~valid] = sigma[named_valid].min() if named_valid.size else np.nan
    ok = {g: None for g, i in col.items() if valid[i] or not only_valid}
    goi = list(ok) if genes is None else [x for x in genes if x in ok]
    if len(goi) == 0:
        raise ValueError("None of the input genes are valid! Genes should be valid as given in geneStats attribute")
    idx = np.array([col[g] for g in goi], dtype=np.int64)
    return goi, mu[idx], sigma[idx]


def _as_params(names, mu, sigma):
    """a pandas DataFrame indexed by gene with columns mu and sigma when pandas can be imported, else a dict"""
    try:
        import pandas as pd
    except ImportError:
        return {"genes": list(names), "mu": mu, "sigma": sigma}
    return pd.DataFrame({"mu": mu, "sigma": sigma, "genes": list(names)}).set_index("genes")


def _params(scaling_params):
    """(names, mu, sigma) of either form get_scaling_params returns"""
    if isinstance(scaling_params, dict):
        names, mu, sigma = list(scaling_params["genes"]), scaling_params["mu"], scaling_params["sigma"]
    else:
        names, mu, sigma = list(scaling_params.index), scaling_params["mu"].values, scaling_params["sigma"].values
    names = [str(x) for x in names]
    if len(set(names)) != len(names):
        seen = set()
        twice = [x for x in names if x in seen or seen.add(x)]
        raise ValueError("ERROR: scaling_params names gene %s twice" % twice[0])
    return names, np.asarray(mu, dtype=np.float64), np.asarray(sigma, dtype=np.float64)


def _gene_pos(raw_genes, names, fill_missing):
    """position of every raw gene among `names` or -1 (get_scaled_values :872-903): a name the file holds twice maps
    through its last index, as geneIdx does; a name the file lacks raises KeyError unless fill_missing"""
    gene_idx = {x: n for n, x in enumerate(raw_genes)}
    pos = np.full(len(raw_genes), -1, dtype=np.int32)
    missing = 0
    for n, x in enumerate(names):
        if x not in gene_idx:
            if fill_missing is False:
                raise KeyError("ERROR: Gene name %s not found! 'scaling_params' may come from a Dataset that was not processed by the "
                               "same pipeline; intersect the gene names first, or set 'fill_missing' to True (the gene then counts as 0 "
                               "in every cell)" % x)
            missing += 1
        else:
            pos[gene_idx[x]] = n
    if missing > 0:
        print("WARNING: %d out %d genes are missing in this dataset" % (missing, len(names)))
    return pos


def _project_from_csr(raw_genes, m, rows, transformer, scaling_params, fill_missing=False, step=_device_project):
    """transform_pca on arrays: raw_genes names the genes of the _csr tuple `m`, rows the cells to project.  Returns Z."""
    if transformer is None:
        raise ValueError("ERROR: None value found for transformer. Please make sure that the PCA was fitted")
    if scaling_params is None:
        raise ValueError("ERROR: scaling_params need to be a DataFrame")
    if getattr(transformer, "whiten", False):
        raise ValueError("ERROR: a whitening transformer is not supported (the reference never whitens)")
    names, mu, sigma = _params(scaling_params)
    mean, comps = np.asarray(transformer.mean_, dtype=np.float64), np.asarray(transformer.components_, dtype=np.float64)
    if mean.ndim != 1 or mean.shape[0] != len(names) or comps.ndim != 2 or comps.shape[1] != len(names):
        raise ValueError("ERROR: the transformer was fitted on %s genes, scaling_params names %d" % (mean.shape, len(names)))
    pos = _gene_pos(raw_genes, names, fill_missing)
    return step(m, *_tables(pos, mu, sigma, mean, comps), np.ascontiguousarray(rows, dtype=np.int64))


class FittedPCA(object):
    """An exact PCA of the scaled cells, with the attributes of sklearn's IncrementalPCA that Nabo reads: mean_,
    components_ [C, G], explained_variance_, explained_variance_ratio_ (over the trace of the covariance),
    singular_values_, var_ (the genes' sample variances), n_samples_seen_, n_components_, whiten (False), genes;
    fit_pca adds scaling_params.  transform_pca takes it as its transformer."""
    whiten = False

    def __init__(self, mean, cov, n, n_comps, genes=None):
        mean, cov = np.asarray(mean, dtype=np.float64), np.asarray(cov, dtype=np.float64)
        G, n, n_comps = mean.shape[0], int(n), int(n_comps)
        if cov.shape != (G, G):
            raise ValueError("ERROR: the mean holds %d genes, the covariance has shape %s" % (G, cov.shape))
        if n < 2:
            raise ValueError("ERROR: a PCA needs at least 2 cells, got %d" % n)
        if n_comps < 1 or n_comps > G:
            raise ValueError("ERROR: n_comps=%d must be between 1 and the number of genes, %d" % (n_comps, G))
        lam, vec = np.linalg.eigh(cov)
        lam, vec = lam[::-1][:n_comps], vec[:, ::-1][:, :n_comps]       # descending; equal values in eigh's order, reversed
        comp = np.ascontiguousarray(vec.T)
        # sklearn's svd_flip(u_based_decision=False): the entry of largest magnitude of a component is positive, the first on a tie
        big = np.argmax(np.abs(comp), axis=1)
        sign = np.sign(comp[np.arange(n_comps), big])
        sign[sign == 0] = 1.0
        self.mean_ = mean.copy()
        self.components_ = comp * sign[:, None]
        self.explained_variance_ = np.maximum(lam, 0.0)
        self.var_ = np.diag(cov).copy()
        trace = float(self.var_.sum())
        self.explained_variance_ratio_ = self.explained_variance_ / trace if trace > 0 else np.zeros(n_comps)
        self.singular_values_ = np.sqrt(self.explained_variance_ * (n - 1))
        self.n_samples_seen_ = n
        self.n_components_ = self.n_components = n_comps
        self.genes = None if genes is None else list(genes)

    def transform(self, X):
        """dense rows X[., G] of scaled values -> their coordinates [., C] (numpy, for small checks)"""
        return (np.asarray(X, dtype=np.float64) - self.mean_) @ self.components_.T


def _reset_n_comps(n_comps, n_genes_asked, n_kept_cells):
    """the two resets of fit_ipca (nabo/_dataset.py:943-951), with its warnings"""
    n_comps = int(n_comps)
    if n_genes_asked < n_comps:
        n_comps = n_genes_asked
        print("WARNING: Number of components were reset to number of features i.e. %d" % n_comps)
    if n_comps > n_kept_cells:
        n_comps = n_kept_cells - 1
        print("WARNING: Number of components were reset to number of cells - 1 i.e. %d" % n_comps)
    return n_comps


def _fit_from_csr(raw_genes, m, rows, scaling_params, n_comps, fill_missing=False, step=_device_cov):
    """fit_ipca on arrays, exactly: raw_genes names the genes of the _csr tuple `m`, rows the cells to fit on.  Returns a
    FittedPCA over the genes of scaling_params."""
    if scaling_params is None:
        raise ValueError("ERROR: scaling_params need to be a DataFrame")
    names, mu, sigma = _params(scaling_params)
    rows = np.ascontiguousarray(rows, dtype=np.int64)
    if rows.ndim != 1 or rows.shape[0] < 2:
        raise ValueError("ERROR: a PCA needs at least 2 cells, got %s" % (rows.shape,))
    if int(n_comps) < 1 or int(n_comps) > len(names):
        raise ValueError("ERROR: n_comps=%d must be between 1 and the number of genes, %d" % (int(n_comps), len(names)))
    pos = _gene_pos(raw_genes, names, fill_missing)
    mean, cov = step(m, *_fit_tables(pos, mu, sigma), rows)
    return FittedPCA(mean, cov, rows.shape[0], n_comps, names)


def fit_pca_csr(cell_ptr, gene, val, sf, gene_pos, mu, sigma, n_comps, rows=None, mem_budget=0, device=0):
    """An exact PCA of the scaled cells: pca_cov_csr on the MI355X, then numpy.linalg.eigh of the G x G covariance on the
    host.  Arguments as for pca_cov_csr.  Returns a FittedPCA with the n_comps leading components."""
    m = _csr((cell_ptr, gene, val, sf))
    rows = _index_list(rows, "rows")
    mean, cov = _device_cov(m, *_fit_tables(gene_pos, mu, sigma), rows, mem_budget, device)
    return FittedPCA(mean, cov, m[0] if rows is None else rows.shape[0], n_comps)


# ---- the Nabo dataset file ----------------------------------------------------------------------------------------
def get_scaling_params(dataset_h5, genes=None, only_valid=True, device=0):
    """Dataset.get_scaling_params (nabo/_dataset.py:814-844, over set_gene_stats :594-637) on a Nabo dataset file: the
    genes' mean `mu` and standard deviation `sigma` (uncorrected, population) of the normalised values over the kept
    cells, for the valid genes in file order or the valid ones among `genes` in the given order.  Raises the
    reference's ValueError when none is valid.  Returns a pandas DataFrame indexed by gene with columns mu and sigma
    when pandas can be imported, otherwise a dict with "genes", "mu" and "sigma".  Deviation: the sums are float64
    over the float32 values (the reference reduces in float32)."""
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

    def step(*a):
        return _device_stats(*a, device=device)
    return _as_params(*_scaling_from_csc(raw_genes, keep_genes_idx, m, keep_cells, genes, only_valid, step))


def transform_pca(dataset_h5, out_file, pca_group_name, transformer, scaling_params, fill_missing=False, layout="cells", mem_budget=0,
                  device=0):
    """Dataset.transform_pca (nabo/_dataset.py:985-1033) on a Nabo dataset file: scales the kept cells with
    `scaling_params` (either form get_scaling_params returns), projects them with `transformer` (any object with
    `mean_` and `components_`: what fit_pca returns, or sklearn's IncrementalPCA) on the MI355X and writes the vectors to group
    `pca_group_name` of `out_file`, replacing the group if it exists.  layout "cells" writes the reference's one dataset
    per cell, "dense" one matrix (write_dense_pca); `Mapping` reads both.  A gene of scaling_params the file lacks
    raises KeyError, or counts as 0 in every cell with fill_missing=True (with the reference's warning).  Deviations: a
    whitening transformer, a gene named twice and a sigma that is not finite and > 0 raise ValueError."""
    from ._mapping import _h5py, _write_rows, write_dense_pca
    if layout not in ("cells", "dense"):
        raise ValueError("ERROR: layout must be 'cells' or 'dense'")
    if transformer is None:
        raise ValueError("ERROR: None value found for transformer. Please make sure that the PCA was fitted")
    if scaling_params is None:
        raise ValueError("ERROR: scaling_params need to be a DataFrame")
    d = _DatasetFile(dataset_h5)
    try:
        rows = np.array(d.keep_cells_idx, dtype=np.int64)
        raw_genes, names = d.genes, [d.cells[i] for i in d.keep_cells_idx]
        m = _csr(d.csr(d.keep_cells_idx))
    finally:
        d.close()

    def step(*a):
        return _device_project(*a, mem_budget=mem_budget, device=device)
    Z = _project_from_csr(raw_genes, m, rows, transformer, scaling_params, fill_missing, step)
    if layout == "dense":
        write_dense_pca(out_file, pca_group_name, names, Z)
        return None
    try:
        h5 = _h5py().File(out_file, mode="a")
    except Exception:
        raise IOError("ERROR: Could not open file %s" % out_file)
    try:
        if pca_group_name in h5:
            del h5[pca_group_name]
        _write_rows(h5.create_group(pca_group_name), names, Z)
    finally:
        h5.close()
    return None


def fit_pca(dataset_h5, genes, n_comps=100, batch_size=None, fill_missing=False, mem_budget=0, device=0):
    """Dataset.fit_ipca (nabo/_dataset.py:917-983) on a Nabo dataset file, as an exact fit: the scaling parameters of
    `genes` from get_scaling_params, mean and covariance of the kept cells' scaled values on the MI355X, the
    eigen-decomposition on the host.  Returns a FittedPCA with `.scaling_params` (what get_scaling_params returned) and
    `.genes = list(scaling_params.index)`; transform_pca takes both.  The reference's two resets of n_comps (to
    len(genes), then to the number of kept cells - 1) apply, with its warnings.  `batch_size` is accepted and ignored: the
    reference's IncrementalPCA depends on its batches and is approximate when n_comps < len(genes); this fit is exact and
    has no batches."""
    d = _DatasetFile(dataset_h5)
    try:
        rows = np.array(d.keep_cells_idx, dtype=np.int64)
        raw_genes = d.genes
        m = _csr(d.csr(d.keep_cells_idx))
    finally:
        d.close()
    n_comps = _reset_n_comps(n_comps, len(genes), rows.shape[0])
    sp = get_scaling_params(dataset_h5, genes, device=device)

    def step(*a):
        return _device_cov(*a, mem_budget=mem_budget, device=device)
    fit = _fit_from_csr(raw_genes, m, rows, sp, n_comps, fill_missing, step)
    fit.scaling_params = sp
    return fit
