"""What the expression-matrix steps (_qc, _pca, _de) share on the Python side: the checks of a matrix given as compressed
sparse rows of cells or columns of genes, of an index list, and the reader of a Nabo dataset file.
"""
import numpy as np


def int32(a, what):
    a = np.asarray(a)
    if a.size and (a.min() < -2 ** 31 or a.max() >= 2 ** 31):
        raise ValueError("ERROR: %s: an index does not fit 32 bits" % what)
    return np.ascontiguousarray(a, dtype=np.int32)


def csr(m):
    """(n_cells, cell_ptr int64, gene int32, val float32, sf float32) from (cell_ptr, gene, val, sf); without size factors
    (cell_ptr int64, gene int32, val float32) from (cell_ptr, gene, val)"""
    with_sf = len(m) == 4
    cell_ptr = np.ascontiguousarray(m[0], dtype=np.int64)
    gene = int32(m[1], "gene")
    val = np.ascontiguousarray(m[2], dtype=np.float32)
    sf = np.ascontiguousarray(m[3], dtype=np.float32) if with_sf else None
    if cell_ptr.ndim != 1 or gene.ndim != 1 or val.ndim != 1 or (with_sf and sf.ndim != 1) or cell_ptr.shape[0] < 1:
        raise ValueError("ERROR: cell_ptr, gene%s must be 1-D, cell_ptr with n_cells + 1 entries" % (", val and sf" if with_sf else " and val"))
    if with_sf and sf.shape[0] != cell_ptr.shape[0] - 1:
        raise ValueError("ERROR: cell_ptr describes %d cells, sf holds %d" % (cell_ptr.shape[0] - 1, sf.shape[0]))
    if gene.shape != val.shape or int(cell_ptr[-1]) != gene.shape[0]:
        raise ValueError("ERROR: cell_ptr[-1] = %d, gene has %d and val %d entries" % (int(cell_ptr[-1]), gene.shape[0], val.shape[0]))
    return (sf.shape[0], cell_ptr, gene, val, sf) if with_sf else (cell_ptr, gene, val)


def csc(m, what):
    """(n_cells, gene_ptr int64, cell int32, val float32, sf float32) from (gene_ptr, cell, val, sf)"""
    gene_ptr, cell, val, sf = m
    gene_ptr = np.ascontiguousarray(gene_ptr, dtype=np.int64)
    cell_in = np.asarray(cell)
    if cell_in.size and (cell_in.min() < -2 ** 31 or cell_in.max() >= 2 ** 31):
        raise ValueError("ERROR: %s: a cell index does not fit 32 bits" % what)
    cell = np.ascontiguousarray(cell_in, dtype=np.int32)
    val, sf = np.ascontiguousarray(val, dtype=np.float32), np.ascontiguousarray(sf, dtype=np.float32)
    if gene_ptr.ndim != 1 or cell.ndim != 1 or val.ndim != 1 or sf.ndim != 1 or gene_ptr.shape[0] < 1:
        raise ValueError("ERROR: %s: gene_ptr, cell, val and sf must be 1-D, gene_ptr with n_genes + 1 entries" % what)
    if cell.shape != val.shape or int(gene_ptr[-1]) != cell.shape[0]:
        raise ValueError("ERROR: %s: gene_ptr[-1] = %d, cell has %d and val %d entries" % (what, int(gene_ptr[-1]), cell.shape[0], val.shape[0]))
    return sf.shape[0], gene_ptr, cell, val, sf


def index_list(a, what):
    if a is None:
        return None
    a = np.ascontiguousarray(a, dtype=np.int64)
    if a.ndim != 1:
        raise ValueError("ERROR: %s must be 1-D" % what)
    return a


def ptr(a):
    """the address of an index list for the C ABI, where NULL means 'all': None -> NULL, an empty list -> not NULL"""
    if a is None:
        return None
    return a.ctypes.data if a.shape[0] else np.zeros(1, dtype=np.int64).ctypes.data


class DatasetFile:
    """what the reference's Dataset reads of a Nabo HDF5 file for this path (nabo/_dataset.py:87-127, 165-206): cell and
    gene names, the kept genes (all, when the file names none), the size factors (ones, when it holds none) and a
    gene's (idx, val) column.  Opened read-only; the reference's Dataset creates `processed_data` when it is missing."""

    def __init__(self, fn):
        import h5py
        self.h5 = h5py.File(fn, "r")
        self.cells = [x.decode("UTF-8") for x in self.h5["names"]["cells"][:]]
        self.genes = [x.decode("UTF-8") for x in self.h5["names"]["genes"][:]]
        self.cell_idx = {x: n for n, x in enumerate(self.cells)}
        grp = self.h5["processed_data"] if "processed_data" in self.h5 else {}
        self.keep_genes_idx = [int(x) for x in grp["keep_genes_idx"][:]] if "keep_genes_idx" in grp else list(range(len(self.genes)))
        self.keep_cells_idx = [int(x) for x in grp["keep_cells_idx"][:]] if "keep_cells_idx" in grp else list(range(len(self.cells)))
        if "sf" in grp:
            self.sf = grp["sf"][:]
            if self.sf.dtype != np.float32:
                raise ValueError("ERROR: processed_data/sf is %s; Nabo writes float32 size factors and the values are "
                                 "defined as float32 products" % self.sf.dtype)
        else:
            self.sf = np.ones(len(self.cells), dtype=np.float32)

    def close(self):
        self.h5.close()

    @staticmethod
    def _record(d):
        """(idx int64 strictly increasing, val float32) of an (idx, val) record; an index listed twice keeps its last
        value, as the reference's scatter does"""
        idx, val = np.asarray(d["idx"], dtype=np.int64), np.asarray(d["val"], dtype=np.float32)
        if idx.shape[0] > 1 and (np.diff(idx) <= 0).any():
            last = {int(c): k for k, c in enumerate(idx.tolist())}
            keep = np.array(sorted(last.values()), dtype=np.int64)
            idx, val = idx[keep], val[keep]
            o = np.argsort(idx, kind="stable")
            idx, val = idx[o], val[o]
        return idx, val

    def csr(self, cells_idx):
        """(cell_ptr int64, gene int32, val float32, sf) over ALL cells of the file, from the `cell_data/<cell>` records
        (nabo/_dataset.py:906-908): the rows of `cells_idx` are read, every other row is empty"""
        n = len(self.cells)
        counts = np.zeros(n, dtype=np.int64)
        got = {}
        cd = self.h5["cell_data"]
        for i in dict.fromkeys(int(x) for x in cells_idx):
            got[i] = self._record(cd[self.cells[i]][:])
            counts[i] = got[i][0].shape[0]
        order = sorted(got)
        ptr = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(counts, out=ptr[1:])
        gene = np.concatenate([got[i][0] for i in order] + [np.zeros(0, np.int64)])
        if gene.size and (gene.min() < 0 or gene.max() >= len(self.genes)):
            raise ValueError("ERROR: cell_data holds a gene index outside [0, %d)" % len(self.genes))
        return ptr, gene.astype(np.int32), np.concatenate([got[i][1] for i in order] + [np.zeros(0, np.float32)]), self.sf

    def csc(self, genes, upper=True):
        """the columns of `genes` as a csc tuple.  A cell listed twice in a column keeps its last value, as the
        reference's scatter does.  `upper`: look the names up in upper case, as get_norm_exp does (:186)."""
        ptr, cells, vals = [0], [], []
        gd = self.h5["gene_data"]
        for g in genes:
            try:
                d = gd[g.upper() if upper else g][:]
            except KeyError:
                raise KeyError("ERROR: This gene symbol does not exist in the dataset.")
            idx, val = self._record(d)
            cells.append(idx)
            vals.append(val)
            ptr.append(ptr[-1] + idx.shape[0])
        return csc((np.array(ptr, dtype=np.int64), np.concatenate(cells) if cells else np.zeros(0, np.int64),
                    np.concatenate(vals) if vals else np.zeros(0, np.float32), self.sf), "the dataset")
