"""Raw counts out and across: Matrix Market text from the cell index, and the remap behind subsetting and merging count
matrices, on the MI355X.

The reference's three functions on raw counts beside mtx_to_h5 are Python loops over one HDF5 dataset per cell and per gene
(nabo/_io.py): `h5_to_mtx` (:645-674) formats one text line per entry, `extract_cells_from_h5` (:597-642) and `merge_h5`
(:502-594) pass every index through a Python dict.  Here the text is formatted by `nabo_mtxw_*` and the indexes are
renumbered, regrouped and rebuilt by `nabo_counts_remap` (include/nabo_counts.h, nabo_amd/csrc/counts.hip); the three
file-level functions keep the reference's signatures and read and write the same dataset files.
"""
import ctypes as C
import gzip
import os

import numpy as np

from . import _lib
from ._ingest import CountMatrix, write_dataset_file

READ_BYTES = 16 << 20               # what write_mtx takes from the writer at a time
H5_TO_MTX_COMMENT = '%metadata_json: {"format_version": 2, "software_version": "3.0.2"}\n'


def writer_geometry():
    """{"tile_bytes": the text one workgroup formats, "min_chunk": the smallest chunk_bytes, "long_cell": a cell of more
    entries gets a workgroup in the length pass, "max_line": the longest line} (nabo_mtxw_geometry)"""
    v = [C.c_int32() for _ in range(4)]
    _lib.check(_lib.lib().nabo_mtxw_geometry(*[C.byref(x) for x in v]))
    return dict(zip(("tile_bytes", "min_chunk", "long_cell", "max_line"), [int(x.value) for x in v]))


def _u32_values(val, what="values"):
    """integer values in [0, 2^32) as uint32; anything else is a ValueError"""
    a = np.asarray(val)
    if a.dtype == np.uint32:
        return np.ascontiguousarray(a)
    if a.dtype.kind == "f":
        if a.size and not (np.isfinite(a).all() and (a == np.floor(a)).all()):
            raise ValueError("ERROR: %s must be integers" % what)
    elif a.dtype.kind not in "iub":
        raise ValueError("ERROR: %s must be integers" % what)
    if a.size and (a.min() < 0 or a.max() > 0xFFFFFFFF):
        raise ValueError("ERROR: %s must lie in [0, 2^32)" % what)
    return np.ascontiguousarray(a.astype(np.uint32))


def _cell_index(m):
    """(cell_ptr int64, gene int32, val uint32) of a CountMatrix or of a (cell_ptr, gene, val) tuple"""
    if isinstance(m, CountMatrix):
        m = (m.cell_ptr, m.gene, m.val)
    ptr, idx, val = m
    ptr, idx = np.ascontiguousarray(ptr, dtype=np.int64), np.ascontiguousarray(idx, dtype=np.int32)
    val = _u32_values(val)
    if ptr.ndim != 1 or ptr.shape[0] < 1 or idx.ndim != 1 or val.shape != idx.shape:
        raise ValueError("ERROR: a matrix is (ptr [n + 1], idx [nnz], val [nnz])")
    return ptr, idx, val


def _p(a):
    return a.ctypes.data if a.size else None


class MtxWriter:
    """The handle of the writer (include/nabo_counts.h): the text of the matrix, byte for byte what `"%d %d %d\\n"` gives,
    in reads of any size.  m: a CountMatrix or (cell_ptr, gene, val) with integer values in [0, 2^32); n_genes is needed
    with a tuple.  comments: None, or whole lines that each start with '%' and end in a newline.  chunk_bytes: the text
    formatted on the device at a time (0: 64 MiB); mem_budget: device bytes (0: three quarters of what is free).
    total_bytes is exact from the start.  Bad input raises ValueError before any device is touched."""

    def __init__(self, m, n_genes=None, comments=None, blank_line_for_empty_cell=False, chunk_bytes=0, mem_budget=0, device=0):
        self._h = C.c_void_p()
        self._lib = _lib.lib()
        if n_genes is None:
            if not isinstance(m, CountMatrix):
                raise ValueError("ERROR: n_genes is needed with a (cell_ptr, gene, val) tuple")
            n_genes = m.n_genes
        ptr, gene, val = _cell_index(m)
        if comments is not None and not isinstance(comments, bytes):
            comments = str(comments).encode("UTF-8")
        total = C.c_int64()
        _lib.check(self._lib.nabo_mtxw_create(int(device), int(n_genes), ptr.shape[0] - 1, ptr.ctypes.data, _p(gene), _p(val), comments,
                                              int(bool(blank_line_for_empty_cell)), int(chunk_bytes), int(mem_budget), C.byref(self._h), C.byref(total)))
        self.total_bytes = int(total.value)

    def readinto(self, buf):
        """the next bytes into a contiguous uint8 array; returns how many (less than its size only at the end, 0 there)"""
        if not (isinstance(buf, np.ndarray) and buf.dtype == np.uint8 and buf.flags.c_contiguous and buf.size > 0):
            raise ValueError("ERROR: readinto takes a contiguous array of uint8 with room for a byte")
        n = C.c_int64()
        _lib.check(self._lib.nabo_mtxw_read(self._h, buf.ctypes.data, buf.size, C.byref(n)))
        return int(n.value)

    def read(self, cap=READ_BYTES):
        """the next bytes, at most cap (>= 1); b"" at the end"""
        buf = np.empty(max(int(cap), 1), dtype=np.uint8)
        return buf[:self.readinto(buf)].tobytes()

    def last_device_ms(self):
        """({"upload", "lengths", "format", "download"} in ms between HIP events, chunks formatted)"""
        ms, chunks = (C.c_double * 4)(), C.c_int64()
        _lib.check(self._lib.nabo_mtxw_last_device_ms(self._h, ms, C.byref(chunks)))
        return dict(zip(("upload", "lengths", "format", "download"), [float(x) for x in ms])), int(chunks.value)

    def close(self):
        if self._h:
            self._lib.nabo_mtxw_free(self._h)
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


def write_mtx(m, target, comments=None, blank_line_for_empty_cell=False, n_genes=None, chunk_bytes=0, mem_budget=0, device=0):
    """Write the counts as Matrix Market text, formatted on the MI355X; returns the number of bytes of text.

    m: a CountMatrix, or a (cell_ptr, gene, val) tuple with integer values in [0, 2^32) and n_genes given.  target: a
    file name (one that ends in `.gz` is deflated on the host by Python's gzip: such a write is bound by the host's
    deflate, not by the formatter), a directory (`matrix.mtx` in it), or an object with write(bytes).  The text: the
    banner, `comments`, the size line, and one line `gene cell value` (1-based) per entry, cells in order and genes
    ascending inside a cell; with blank_line_for_empty_cell a cell without entries leaves an empty line, as the
    reference's h5_to_mtx does.  read_mtx of the text gives m back."""
    if hasattr(target, "write"):
        f, own = target, False
    else:
        fn = str(target)
        if os.path.isdir(fn):
            fn = os.path.join(fn, "matrix.mtx")
        f, own = (gzip.open(fn, "wb") if fn.endswith(".gz") else open(fn, "wb")), True
    try:
        with MtxWriter(m, n_genes, comments, blank_line_for_empty_cell, chunk_bytes, mem_budget, device) as w:
            buf = np.empty(max(min(READ_BYTES, w.total_bytes), 1), dtype=np.uint8)
            while True:
                n = w.readinto(buf)
                if n == 0:
                    break
                f.write(memoryview(buf[:n]))
            return w.total_bytes
    finally:
        if own:
            f.close()


def remap_counts(ptr, idx, val, n_cols, row_src, col_map, n_out_cols, with_csc=True, device=0):
    """The array level of nabo_counts_remap: output row r is input row row_src[r] (repeats allowed), column j becomes
    col_map[j], columns with col_map -1 are dropped.  val: uint32 or float32, kept bit for bit in its dtype.  Returns
    (out_ptr int64, out_idx int32 strictly increasing inside a row, out_val) and, with_csc, (csc_ptr int64 [n_out_cols +
    1], csc_idx int32 -- the rows, strictly increasing inside a column --, csc_val) as a second tuple (None without).
    Two kept columns of one row that map to the same output column raise ValueError, with the lowest such (row, column);
    so does any bad argument, before any device is touched."""
    ptr, idx = np.ascontiguousarray(ptr, dtype=np.int64), np.ascontiguousarray(idx, dtype=np.int32)
    val = np.ascontiguousarray(val)
    if val.dtype not in (np.dtype(np.uint32), np.dtype(np.float32)):
        raise ValueError("ERROR: val must be uint32 or float32")
    if ptr.ndim != 1 or ptr.shape[0] < 1 or idx.ndim != 1 or val.shape != idx.shape:
        raise ValueError("ERROR: a matrix is (ptr [n + 1], idx [nnz], val [nnz])")
    row_src, col_map = np.ascontiguousarray(row_src, dtype=np.int64), np.ascontiguousarray(col_map, dtype=np.int32)
    n_rows, n_cols, n_out_rows, n_out_cols = ptr.shape[0] - 1, int(n_cols), row_src.shape[0], int(n_out_cols)
    if row_src.ndim != 1 or col_map.shape != (max(n_cols, 0),):
        raise ValueError("ERROR: row_src must be one-dimensional and col_map hold one entry per input column")
    # the bound of the header; a bad ptr or row_src is refused by the library, with its message
    ok = n_rows > 0 and ptr[0] == 0 and (np.diff(ptr) >= 0).all() and row_src.size > 0 and row_src.min() >= 0 and row_src.max() < n_rows
    bound = int(np.diff(ptr)[row_src].sum()) if ok else 0
    if ptr[-1] != idx.shape[0]:
        raise ValueError("ERROR: ptr[-1] = %d, but there are %d entries" % (int(ptr[-1]), idx.shape[0]))
    out_ptr, out_idx, out_val = np.zeros(n_out_rows + 1, np.int64), np.zeros(bound, np.int32), np.zeros(bound, val.dtype)
    csc = (np.zeros(max(n_out_cols, 0) + 1, np.int64), np.zeros(bound, np.int32), np.zeros(bound, val.dtype)) if with_csc else None
    one, nnz = np.zeros(2, np.int64), C.c_int64()
    at = lambda a: a.ctypes.data if a.size else one.ctypes.data  # noqa: E731
    _lib.check(_lib.lib().nabo_counts_remap(int(device), n_rows, n_cols, ptr.ctypes.data, at(idx), at(val), n_out_rows, at(row_src), n_out_cols,
                                            at(col_map), C.byref(nnz), out_ptr.ctypes.data, at(out_idx), at(out_val),
                                            csc[0].ctypes.data if csc else None, at(csc[1]) if csc else None, at(csc[2]) if csc else None))
    n = int(nnz.value)
    return (out_ptr, out_idx[:n].copy(), out_val[:n].copy()), ((csc[0], csc[1][:n].copy(), csc[2][:n].copy()) if csc else None)


def _count_matrix(n_genes, csr, csc):
    return CountMatrix(n_genes, csr[0].shape[0] - 1, csr[0], csr[1], csr[2], csc[0], csc[1], csc[2])


def subset_cells(m, rows, device=0):
    """The CountMatrix of the cells `rows` of m, in the order given (repeats allowed), over all genes of m."""
    csr, csc = remap_counts(m.cell_ptr, m.gene, m.val, m.n_genes, rows, np.arange(m.n_genes, dtype=np.int32), m.n_genes, device=device)
    return _count_matrix(m.n_genes, csr, csc)


def merge_counts(matrices, gene_names, cell_names, cell_suffixes=None, cell_order=None, seed=0, device=0):
    """Pool count matrices: (CountMatrix, genes, cells).

    matrices: CountMatrix objects; gene_names and cell_names: one list of names per matrix.  The genes of the result are
    the SORTED UNION of all gene names (every gene name must be unique within its matrix); the cells are `name + '-' +
    suffix` (cell_suffixes default '1', '2', ...) and must come out distinct.  cell_order: the merged cell names in the
    order wanted (a permutation of them); None: a permutation drawn by numpy's default_rng(seed) -- the reference draws an
    unseeded random.sample.  Records come out ascending by index in both indexes."""
    k = len(matrices)
    if cell_suffixes is None:
        cell_suffixes = [str(x + 1) for x in range(k)]
    elif len(cell_suffixes) != k:
        raise ValueError("ERROR: Number of cell_suffixes not same as number of input H5 files")
    if len(gene_names) != k or len(cell_names) != k:
        raise ValueError("ERROR: one list of gene names and one of cell names per matrix")
    genes = sorted(set(str(g) for names in gene_names for g in names))
    where = {g: n for n, g in enumerate(genes)}
    parts, cells = [], []
    for i, m in enumerate(matrices):
        if len(gene_names[i]) != m.n_genes or len(cell_names[i]) != m.n_cells or len(set(gene_names[i])) != m.n_genes:
            raise ValueError("ERROR: matrix %d: the names do not fit the matrix, or a gene name occurs twice" % i)
        col_map = np.array([where[str(g)] for g in gene_names[i]], dtype=np.int32).reshape(-1)
        parts.append(remap_counts(m.cell_ptr, m.gene, m.val, m.n_genes, np.arange(m.n_cells, dtype=np.int64), col_map, len(genes), with_csc=False,
                                  device=device)[0])
        cells.extend(str(c) + "-" + str(cell_suffixes[i]) for c in cell_names[i])
    if len(set(cells)) != len(cells):
        raise ValueError("ERROR: the merged cell names are not distinct")
    if cell_order is None:
        order = np.random.default_rng(seed).permutation(len(cells)).astype(np.int64)
    else:
        at = {c: n for n, c in enumerate(cells)}
        if len(cell_order) != len(cells) or set(cell_order) != set(cells):
            raise ValueError("ERROR: cell_order must be a permutation of the merged cell names")
        order = np.array([at[str(c)] for c in cell_order], dtype=np.int64).reshape(-1)
    ptr = np.zeros(len(cells) + 1, dtype=np.int64)
    np.cumsum(np.concatenate([np.diff(p[0]) for p in parts] + [np.zeros(0, np.int64)]), out=ptr[1:])
    idx = np.concatenate([p[1] for p in parts] + [np.zeros(0, np.int32)])
    val = np.concatenate([p[2] for p in parts] + [np.zeros(0, np.uint32)])
    csr, csc = remap_counts(ptr, idx, val, len(genes), order, np.arange(len(genes), dtype=np.int32), len(genes), device=device)
    return _count_matrix(len(genes), csr, csc), genes, [cells[i] for i in order.tolist()]


# ---- the dataset file -----------------------------------------------------------------------------------------------
REQUIRED_KEYS = ("gene_data", "cell_data", "names/cells", "names/genes")


def _read_h5(fn, device=0):
    """(CountMatrix, genes, cells, the file's value dtype)"""
    import h5py
    with h5py.File(fn, "r") as h5:
        genes = [x.decode("UTF-8") for x in h5["names/genes"][:]]
        cells = [x.decode("UTF-8") for x in h5["names/cells"][:]]
        grp, recs, value_dtype = h5["cell_data"], [], np.dtype(np.int64)
        for c in cells:
            if c in grp:
                r = grp[c][:]
                value_dtype = r.dtype["val"]
                if r.shape[0] > 1 and not (np.diff(r["idx"].astype(np.int64)) > 0).all():
                    r = r[np.argsort(r["idx"], kind="stable")]
                recs.append(r)
            else:
                recs.append(None)
    ptr = np.zeros(len(cells) + 1, dtype=np.int64)
    np.cumsum([0 if r is None else r.shape[0] for r in recs], out=ptr[1:])
    have = [r for r in recs if r is not None and r.shape[0]]
    idx = np.concatenate([r["idx"] for r in have]).astype(np.int32) if have else np.zeros(0, np.int32)
    raw = np.concatenate([r["val"] for r in have]) if have else np.zeros(0, np.int64)
    val = _u32_values(raw, "the values of %s" % fn)
    csr, csc = remap_counts(ptr, idx, val, len(genes), np.arange(len(cells), dtype=np.int64), np.arange(len(genes), dtype=np.int32), len(genes),
                            device=device)
    return _count_matrix(len(genes), csr, csc), genes, cells, value_dtype


def read_h5_counts(fn, device=0):
    """(CountMatrix, genes, cells) of a Nabo dataset file, read from its cell_data (a cell without a dataset has no
    entries); the gene index is rebuilt on the device.  Values that are not integers in [0, 2^32) raise ValueError."""
    return _read_h5(fn, device)[:3]


def _fresh(fn):
    if os.path.isfile(fn):
        os.remove(fn)
    return fn


def extract_cells_from_h5(in_fn, out_fn, coi):
    """The reference's extract_cells_from_h5 (nabo/_io.py:597-642): the cells named in coi, in the order of the FILE, with
    all genes, to a new dataset file.  None of them found: the reference's ValueError; some: its WARNING line.  Records
    keep the input's value dtype.  The subset is cut by nabo_counts_remap; an existing out_fn is overwritten."""
    m, genes, cells, value_dtype = _read_h5(in_fn)
    coi = {x: None for x in coi}
    rows = [n for n, c in enumerate(cells) if c in coi]
    if len(rows) == 0:
        raise ValueError("ERROR: None of the input cells were found in the H5 file")
    if len(rows) != len(coi):
        print("WARNING: only %d/%d cells found in the H5 file" % (len(rows), len(coi)))
    write_dataset_file(_fresh(out_fn), subset_cells(m, np.array(rows, dtype=np.int64)), genes, [cells[r] for r in rows], value_dtype)
    return None


def merge_h5(h5_fns, merged_fn, cell_suffixes=None, cell_order=None, seed=0):
    """The reference's merge_h5 (nabo/_io.py:502-594): pool dataset files into one.  The reference's errors: KeyError for
    a file without one of its four groups, ValueError for a wrong number of cell_suffixes.  Departures, all stated in
    merge_counts: the genes are the sorted union over ALL files (the reference's `union_genes.union(...)` discards its
    result, so it raises KeyError as soon as a later file has a gene the first lacks; with equal gene sets the two agree);
    the default cell order is a seeded permutation (the reference's is an unseeded random.sample; cell_order reproduces
    any); records are ascending by index (the reference leaves gene records in concatenation order)."""
    import h5py
    for fn in h5_fns:
        with h5py.File(fn, "r") as h5:
            for key in REQUIRED_KEYS:
                if key not in h5:
                    raise KeyError("ERROR: Group %s missing in file %s" % (key, fn))
    if cell_suffixes is not None and len(cell_suffixes) != len(h5_fns):
        raise ValueError("ERROR: Number of cell_suffixes not same as number of input H5 files")
    read = [_read_h5(fn) for fn in h5_fns]
    m, genes, cells = merge_counts([r[0] for r in read], [r[1] for r in read], [r[2] for r in read], cell_suffixes, cell_order, seed)
    write_dataset_file(_fresh(merged_fn), m, genes, cells, read[0][3] if read else np.int64)
    return None


def h5_to_mtx(fn, outdir):
    """The reference's h5_to_mtx (nabo/_io.py:645-674): a dataset file to outdir/matrix.mtx, genes.tsv (`name<TAB>name`)
    and barcodes.tsv.  The text is the reference's byte for byte: its two header lines (the banner and its
    `%metadata_json` line), the size line, the entries by cell with genes ascending, an empty line for a cell without
    entries.  Departures: the file is opened read-only (the reference constructs a Dataset with force_recalc, which
    deletes the file's processed_data), and values that are not integers are refused (the reference truncates them)."""
    m, genes, cells = read_h5_counts(fn)
    write_mtx(m, os.path.join(str(outdir), "matrix.mtx"), comments=H5_TO_MTX_COMMENT, blank_line_for_empty_cell=True)
    with open(os.path.join(str(outdir), "genes.tsv"), "w") as h:
        h.write("\n".join([x + "\t" + x for x in genes]) + "\n")
    with open(os.path.join(str(outdir), "barcodes.tsv"), "w") as h:
        h.write("\n".join(cells) + "\n")
    return None
