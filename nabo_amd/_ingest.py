"""Raw counts in: Matrix Market text to the cell index (CSR) and the gene index (CSC) on the MI355X.

The reference's way in is nabo/_io.py's `mtx_to_h5` (:61-235), a Python loop per text line and a Python transpose per
batch of cells.  Here the text is parsed by `nabo_mtx_*` (include/nabo_ingest.h, nabo_amd/csrc/mtx_ingest.hip): the
bytes are fed in chunks, parsed on the device, sorted twice, and come back as the two indexes the array-level entry
points read -- `cell_qc_csr`, `pca_project_csr` and `fit_pca_csr` the rows of cells, `gene_stats_csc` and `de_test_csc`
the columns of genes.  `mtx_to_h5` keeps the reference's signature and writes the same dataset file.
"""
import ctypes as C
import gzip
import os

import numpy as np

from . import _lib
from ._matrixio import csr as _csr

READ_BYTES = 16 << 20               # what read_mtx reads, or inflates, at a time


def geometry():
    """{"tile_bytes": the text one workgroup owns, "max_line": the longest body line accepted} (nabo_mtx_geometry)"""
    t, m = C.c_int32(), C.c_int32()
    _lib.check(_lib.lib().nabo_mtx_geometry(C.byref(t), C.byref(m)))
    return {"tile_bytes": int(t.value), "max_line": int(m.value)}


class CountMatrix:
    """The counts of a Matrix Market file, indexed twice.

    n_genes, n_cells; by cell: cell_ptr int64 [n_cells + 1], gene int32 [nnz], val uint32 [nnz] -- cell c lists the genes
    gene[cell_ptr[c]:cell_ptr[c + 1]], strictly increasing; by gene: gene_ptr int64 [n_genes + 1], cell int32 [nnz],
    gene_val uint32 [nnz] -- gene g lists the cells cell[gene_ptr[g]:gene_ptr[g + 1]], strictly increasing.  A stored zero
    is an entry.  max_value: the largest count; the entry points of this package take float32 values, and a count of
    2**24 or more is NOT exact in float32 -- csr() and csc() convert all the same, so look at max_value first."""

    def __init__(self, n_genes, n_cells, cell_ptr, gene, val, gene_ptr, cell, gene_val):
        self.n_genes, self.n_cells = int(n_genes), int(n_cells)
        self.cell_ptr, self.gene, self.val = cell_ptr, gene, val
        self.gene_ptr, self.cell, self.gene_val = gene_ptr, cell, gene_val

    @property
    def nnz(self):
        return int(self.gene.shape[0])

    @property
    def max_value(self):
        return int(self.val.max()) if self.val.size else 0

    def csr(self, sf=None):
        """(cell_ptr, gene, val float32) or, with size factors [n_cells], (cell_ptr, gene, val float32, sf): what
        cell_qc_csr, pca_project_csr and fit_pca_csr take"""
        m = (self.cell_ptr, self.gene, self.val.astype(np.float32))
        if sf is None:
            return m
        sf = np.ascontiguousarray(sf, dtype=np.float32)
        if sf.shape != (self.n_cells,):
            raise ValueError("ERROR: sf must hold one size factor per cell (%d)" % self.n_cells)
        return m + (sf,)

    def csc(self, sf):
        """(gene_ptr, cell, val float32, sf) with size factors [n_cells]: what gene_stats_csc and de_test_csc take"""
        sf = np.ascontiguousarray(sf, dtype=np.float32)
        if sf.shape != (self.n_cells,):
            raise ValueError("ERROR: sf must hold one size factor per cell (%d)" % self.n_cells)
        return self.gene_ptr, self.cell, self.gene_val.astype(np.float32), sf


class MtxReader:
    """The streaming handle of include/nabo_ingest.h: feed(bytes) in any split, then finish() -> CountMatrix.
    chunk_bytes: the text parsed at a time (0: the library's default, 64 MiB); mem_budget: device bytes (0: three
    quarters of what is free).  A grammar or range error raises ValueError, "ERROR: line N: ..." with the lowest bad
    line of the file."""

    def __init__(self, chunk_bytes=0, mem_budget=0, device=0):
        self._h = C.c_void_p()
        self._lib = _lib.lib()
        _lib.check(self._lib.nabo_mtx_create(int(device), int(chunk_bytes), int(mem_budget), C.byref(self._h)))

    def feed(self, data):
        """the next bytes of the file: bytes, or anything numpy reads as a run of uint8 without a copy"""
        if isinstance(data, bytes):
            _lib.check(self._lib.nabo_mtx_feed(self._h, data, len(data)))
            return
        a = np.ascontiguousarray(np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data)
        if a.dtype != np.uint8:
            raise ValueError("ERROR: feed takes bytes or an array of uint8")
        _lib.check(self._lib.nabo_mtx_feed(self._h, a.ctypes.data if a.size else None, a.size))

    def finish(self):
        ng, nc, nnz = C.c_int64(), C.c_int64(), C.c_int64()
        _lib.check(self._lib.nabo_mtx_finish(self._h, C.byref(ng), C.byref(nc), C.byref(nnz)))
        ng, nc, nnz = int(ng.value), int(nc.value), int(nnz.value)
        cell_ptr, gene, val = np.zeros(nc + 1, np.int64), np.zeros(nnz, np.int32), np.zeros(nnz, np.uint32)
        gene_ptr, cell, gval = np.zeros(ng + 1, np.int64), np.zeros(nnz, np.int32), np.zeros(nnz, np.uint32)
        _lib.check(self._lib.nabo_mtx_get_csr(self._h, cell_ptr.ctypes.data, gene.ctypes.data if nnz else None, val.ctypes.data if nnz else None))
        _lib.check(self._lib.nabo_mtx_get_csc(self._h, gene_ptr.ctypes.data, cell.ctypes.data if nnz else None, gval.ctypes.data if nnz else None))
        return CountMatrix(ng, nc, cell_ptr, gene, val, gene_ptr, cell, gval)

    def last_device_ms(self):
        """({"upload", "parse", "sort", "transpose", "download"} in ms between HIP events, chunks parsed)"""
        ms, chunks = (C.c_double * 5)(), C.c_int64()
        _lib.check(self._lib.nabo_mtx_last_device_ms(self._h, ms, C.byref(chunks)))
        return dict(zip(("upload", "parse", "sort", "transpose", "download"), [float(x) for x in ms])), int(chunks.value)

    def close(self):
        if self._h:
            self._lib.nabo_mtx_free(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _first_existing(directory, names):
    for n in names:
        fn = os.path.join(directory, n)
        if os.path.isfile(fn):
            return fn
    return None


def _open_bytes(fn):
    return gzip.open(fn, "rb") if fn.endswith(".gz") else open(fn, "rb")


def read_mtx(source, chunk_bytes=0, mem_budget=0, device=0):
    """Read a Matrix Market file of counts into a CountMatrix on the MI355X.

    source: a file name (plain or `.gz`), a directory that holds `matrix.mtx` or `matrix.mtx.gz`, or an object with
    read(n) that returns bytes.  A gzipped file is inflated on the host by Python's gzip, READ_BYTES at a time, and fed
    to the device as it comes: such a read is bound by the host's inflate, not by the parser."""
    if hasattr(source, "read"):
        f, own = source, False
    else:
        fn = str(source)
        if os.path.isdir(fn):
            found = _first_existing(fn, ("matrix.mtx", "matrix.mtx.gz"))
            if found is None:
                raise FileNotFoundError("Could not find either either matrix.mtx or matrix.mtx.gz in %s" % fn)
            fn = found
        f, own = _open_bytes(fn), True
    try:
        with MtxReader(chunk_bytes, mem_budget, device) as r:
            while True:
                piece = f.read(READ_BYTES)
                if not piece:
                    break
                r.feed(piece)
            return r.finish()
    finally:
        if own:
            f.close()


def csr_to_csc(ptr, idx, val, n_cols, device=0):
    """The transpose on its own (nabo_csr_transpose): a CSR (ptr, idx strictly increasing inside a row, val float32 finite
    and >= 0) over n_cols columns to (out_ptr int64 [n_cols + 1], out_idx int32 -- the rows, ascending inside a column --
    and out_val float32).  Bad input raises ValueError before any device is touched."""
    ptr, idx, val = _csr((ptr, idx, val))
    n_rows, n_cols, nnz = ptr.shape[0] - 1, int(n_cols), idx.shape[0]
    out_ptr, out_idx, out_val = np.zeros(max(n_cols, 0) + 1, np.int64), np.zeros(nnz, np.int32), np.zeros(nnz, np.float32)
    one = np.zeros(1, np.int64)
    _lib.check(_lib.lib().nabo_csr_transpose(int(device), n_rows, n_cols, ptr.ctypes.data, idx.ctypes.data if nnz else one.ctypes.data,
                                             val.ctypes.data if nnz else one.ctypes.data, out_ptr.ctypes.data,
                                             out_idx.ctypes.data if nnz else one.ctypes.data, out_val.ctypes.data if nnz else one.ctypes.data))
    return out_ptr, out_idx, out_val


# ---- the dataset file ---------------------------------------------------------------------------------------------
def fix_dup_names(names):
    """nabo/_io.py:15-32: the names in upper case; one that then occurs more than once gets _1, _2, ... in order"""
    upper = [str(x).upper() for x in names]
    dup = {}
    for x in upper:
        dup[x] = dup.get(x, 0) + 1
    seen, out = {}, []
    for x in upper:
        if dup[x] > 1:
            seen[x] = seen.get(x, 0) + 1
            x = x + "_" + str(seen[x])
        out.append(x)
    return out


def read_gene_names(in_dir):
    """(names, the file they came from): the second whitespace-separated field of every line of the first file found
    among genes.tsv, genes.tsv.gz, features.tsv, features.tsv.gz, through fix_dup_names"""
    names = ("genes.tsv", "genes.tsv.gz", "features.tsv", "features.tsv.gz")
    fn = _first_existing(in_dir, names)
    if fn is None:
        raise FileNotFoundError("ERROR: Could not file gene/features file")
    with _open_bytes(fn) as f:
        lines = [x for x in f.read().decode("UTF-8").splitlines() if x.strip()]
    return fix_dup_names([x.split()[1] for x in lines]), os.path.basename(fn)


def read_barcodes(in_dir):
    fn = _first_existing(in_dir, ("barcodes.tsv", "barcodes.tsv.gz"))
    if fn is None:
        raise FileNotFoundError("ERROR: Could not barcodes file")
    with _open_bytes(fn) as f:
        return [x.upper() for x in f.read().decode("UTF-8").split("\n") if x != ""]


def mtx_to_h5(in_dir, h5_fn, batch_size=10000, value_dtype=np.int64):
    """The reference's mtx_to_h5 (nabo/_io.py:61-83): a directory with matrix.mtx[.gz], genes.tsv / features.tsv[.gz]
    and barcodes.tsv[.gz] to a Nabo dataset file with names/{genes,cells}, cell_data/<cell> and gene_data/<gene>, records
    of dtype [('idx', np.uint), ('val', value_dtype)].  The matrix is read by read_mtx; batch_size is accepted and
    ignored (nothing is batched here).  An existing h5_fn is overwritten.

    One departure: a cell without entries gets an EMPTY cell_data dataset.  The reference writes none (except for the
    first cell, by an accident of its loop), and its own Dataset then fails on such a cell."""
    import h5py  # noqa: F401  (fail before the matrix is read, not after)
    in_dir = str(in_dir)
    m = read_mtx(in_dir)
    genes, gene_file = read_gene_names(in_dir)
    if len(genes) != m.n_genes:
        raise ValueError("Number of gene in %s not same as in the mtx file" % gene_file)
    cells = read_barcodes(in_dir)
    if len(cells) != m.n_cells:
        raise ValueError("Number of cells in barcodes.tsv not same as in the mtx file")
    if os.path.isfile(h5_fn):
        print("Overwriting %s" % h5_fn, flush=True)
        os.remove(h5_fn)
    write_dataset_file(h5_fn, m, genes, cells, value_dtype)
    return None


def write_dataset_file(h5_fn, m, genes, cells, value_dtype=np.int64, idx_dtype=np.uint):
    """A Nabo dataset file of the CountMatrix m: names/{genes,cells}, cell_data/<cell> and gene_data/<gene>, records of
    dtype [('idx', idx_dtype), ('val', value_dtype)], one dataset per cell and per gene (an empty one for none without
    entries).  What mtx_to_h5, extract_cells_from_h5 and merge_h5 write, and csv_to_h5 with idx_dtype=np.int64 (what the
    reference's records have there)."""
    import h5py
    dtype = [("idx", idx_dtype), ("val", value_dtype)]
    with h5py.File(h5_fn, mode="a", libver="latest") as h5:
        grp = h5.create_group("names")
        grp.create_dataset("genes", chunks=None, data=[x.encode("ascii") for x in genes])
        grp.create_dataset("cells", chunks=None, data=[x.encode("ascii") for x in cells])
        for group, names, ptr, idx, val in (("cell_data", cells, m.cell_ptr, m.gene, m.val), ("gene_data", genes, m.gene_ptr, m.cell, m.gene_val)):
            rec = np.zeros(idx.shape[0], dtype=dtype)
            rec["idx"], rec["val"] = idx, val
            grp = h5.create_group(group)
            for i, name in enumerate(names):
                grp.create_dataset(name, data=rec[ptr[i]:ptr[i + 1]], chunks=None)
    return None
