"""Expression tables in: a dense CSV / TSV of numbers to its non-zero entries by row and by column on the MI355X.

The reference's way in is nabo/_io.py's `csv_to_h5` (:238-477): `str.split` and `np.array(vec, dtype=float)` one line at
a time, then a transpose through Python dicts.  Here the body of the table is parsed by `nabo_csv_*`
(include/nabo_csv.h, nabo_amd/csrc/csv_ingest.hip): the bytes are fed in chunks, every field is converted on the device --
bit-equal to Python's float() -- and the entries come back by row and by column.  Skipped lines, the header line and what
the names mean are handled here, by the reference's rules.  `csv_to_h5` keeps the reference's signature and writes the
same dataset file.

Departures from the reference, all refusals or repairs: numpy 1.26 reads `1_0` as 10 and accepts digits outside ASCII,
this reader refuses both ("ERROR: line N, field M: ..."); a trailing `\\r` is taken off the last column name of a header
with CRLF line ends."""
import ctypes as C
import gzip
import os

import numpy as np

from . import _lib
from ._ingest import CountMatrix, fix_dup_names, write_dataset_file

READ_BYTES = 16 << 20               # what read_csv reads, or inflates, at a time


def geometry():
    """{"tile_bytes": the text one workgroup owns, "max_field": the longest value field the device converts itself,
    "max_name": the longest row name} (nabo_csv_geometry)"""
    t, f, n = C.c_int32(), C.c_int32(), C.c_int32()
    _lib.check(_lib.lib().nabo_csv_geometry(C.byref(t), C.byref(f), C.byref(n)))
    return {"tile_bytes": int(t.value), "max_field": int(f.value), "max_name": int(n.value)}


class CsvCounts(CountMatrix):
    """A CsvMatrix under CountMatrix's names; the values are float64 or int64 as they were read."""

    @property
    def max_value(self):
        return self.val.max().item() if self.val.size else 0


class CsvMatrix:
    """The non-zero entries of a table, indexed twice.

    n_rows, n_cols; by row: row_ptr int64 [n_rows + 1], col int32 [nnz], val float64 or int64 [nnz] -- row r lists the
    columns col[row_ptr[r]:row_ptr[r + 1]], strictly increasing; by column: col_ptr int64 [n_cols + 1], row int32 [nnz],
    col_val [nnz].  row_names: the first field of every line as it stands in the file (a list of str, latin-1 decoded so
    that any byte survives), or None when the lines have no name field."""

    def __init__(self, n_rows, n_cols, row_ptr, col, val, col_ptr, row, col_val, row_names=None):
        self.n_rows, self.n_cols = int(n_rows), int(n_cols)
        self.row_ptr, self.col, self.val = row_ptr, col, val
        self.col_ptr, self.row, self.col_val = col_ptr, row, col_val
        self.row_names = row_names

    @property
    def nnz(self):
        return int(self.col.shape[0])

    def counts(self, genes_in_columns=False):
        """The matrix under CountMatrix's attribute names (cell_ptr, gene, val, gene_ptr, cell, gene_val, csr(), csc()):
        rows are genes and columns cells, or the other way round with genes_in_columns"""
        if genes_in_columns:
            return CsvCounts(self.n_cols, self.n_rows, self.row_ptr, self.col, self.val, self.col_ptr, self.row, self.col_val)
        return CsvCounts(self.n_rows, self.n_cols, self.col_ptr, self.row, self.col_val, self.row_ptr, self.col, self.val)


def _kind(value_dtype):
    dt = np.dtype(value_dtype)
    if dt == np.float64:
        return 0, dt
    if dt == np.int64:
        return 1, dt
    raise ValueError("ERROR: value_dtype must be float (float64) or int (int64)")


class CsvReader:
    """The streaming handle of include/nabo_csv.h for the BODY of a table: feed(bytes) in any split, then finish() ->
    CsvMatrix.  sep: one character; n_cols: the value fields of a line; has_row_names: the first field of a line is a
    name; value_dtype: float or int; null_thresh: values below it are 0; first_line: the lines in front of the body, added
    to the line number of every message; chunk_bytes: the text parsed at a time (0: the library's default, 16 MiB);
    mem_budget: device bytes (0: three quarters of what is free).  A grammar error raises ValueError, "ERROR: line N,
    field M: ..." with the lowest bad (line, field) of the stream."""

    def __init__(self, sep=",", n_cols=1, has_row_names=True, value_dtype=float, null_thresh=None, first_line=0, chunk_bytes=0, mem_budget=0, device=0):
        sep = sep.encode("latin-1") if isinstance(sep, str) else bytes(sep)
        if len(sep) != 1:
            raise ValueError("ERROR: sep must be one byte")
        self._kind, self._dtype = _kind(value_dtype)
        self.n_cols, self.has_row_names = int(n_cols), bool(has_row_names)
        self._h = C.c_void_p()
        self._lib = _lib.lib()
        _lib.check(self._lib.nabo_csv_create(int(device), sep[0], self.n_cols, int(self.has_row_names), self._kind, int(null_thresh is not None),
                                             float(null_thresh) if null_thresh is not None else 0.0, int(chunk_bytes), int(mem_budget), C.byref(self._h)))
        if first_line:
            _lib.check(self._lib.nabo_csv_set_first_line(self._h, int(first_line)))

    def feed(self, data):
        """the next bytes of the body: bytes, or anything numpy reads as a run of uint8 without a copy"""
        if isinstance(data, bytes):
            _lib.check(self._lib.nabo_csv_feed(self._h, data, len(data)))
            return
        a = np.ascontiguousarray(np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data)
        if a.dtype != np.uint8:
            raise ValueError("ERROR: feed takes bytes or an array of uint8")
        _lib.check(self._lib.nabo_csv_feed(self._h, a.ctypes.data if a.size else None, a.size))

    def finish(self):
        nr, nnz = C.c_int64(), C.c_int64()
        _lib.check(self._lib.nabo_csv_finish(self._h, C.byref(nr), C.byref(nnz)))
        nr, nnz, nc = int(nr.value), int(nnz.value), self.n_cols
        row_ptr, col, val = np.zeros(nr + 1, np.int64), np.zeros(nnz, np.int32), np.zeros(nnz, self._dtype)
        col_ptr, row, cval = np.zeros(nc + 1, np.int64), np.zeros(nnz, np.int32), np.zeros(nnz, self._dtype)
        _lib.check(self._lib.nabo_csv_get_rows(self._h, row_ptr.ctypes.data, col.ctypes.data if nnz else None, val.ctypes.data if nnz else None))
        _lib.check(self._lib.nabo_csv_get_cols(self._h, col_ptr.ctypes.data, row.ctypes.data if nnz else None, cval.ctypes.data if nnz else None))
        names = None
        if self.has_row_names:
            off = np.zeros(nr + 1, np.int64)
            _lib.check(self._lib.nabo_csv_get_row_names(self._h, off.ctypes.data, None))
            raw = np.zeros(max(int(off[-1]), 1), np.uint8)
            _lib.check(self._lib.nabo_csv_get_row_names(self._h, None, raw.ctypes.data))
            raw = raw.tobytes()
            names = [raw[off[i]:off[i + 1]].decode("latin-1") for i in range(nr)]
        return CsvMatrix(nr, nc, row_ptr, col, val, col_ptr, row, cval, names)

    def stats(self):
        """{"fields": value fields seen, "entries": entries kept, "converted": fields converted on the device, "deferred":
        fields the device left to the host's strtod / strtoll}"""
        out = (C.c_int64 * 4)()
        _lib.check(self._lib.nabo_csv_stats(self._h, out))
        return dict(zip(("fields", "entries", "converted", "deferred"), [int(x) for x in out]))

    def last_device_ms(self):
        """({"upload", "parse", "transpose", "download"} in ms between HIP events, chunks parsed)"""
        ms, chunks = (C.c_double * 4)(), C.c_int64()
        _lib.check(self._lib.nabo_csv_last_device_ms(self._h, ms, C.byref(chunks)))
        return dict(zip(("upload", "parse", "transpose", "download"), [float(x) for x in ms])), int(chunks.value)

    def close(self):
        if self._h:
            self._lib.nabo_csv_free(self._h)
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


def _clean(name):
    return name.strip('"').strip("'").upper()


def header_names(line, sep):
    """nabo/_io.py:349-350 on the bytes of the header line (without its `\\n`): split at sep, quotes off, upper case; a
    trailing `\\r` is taken off first (the departure)"""
    text = line.decode("latin-1")
    if text.endswith("\r"):
        text = text[:-1]
    return [_clean(x) for x in text.split(sep)]


def column_names(colnames, rownames_given, colname_converter=None):
    """nabo/_io.py:352-369: without given row names the first column name belongs to the name column and is dropped;
    the converter, then fix_dup_names"""
    colnames = list(colnames)
    if not rownames_given:
        colnames = colnames[1:]
    if colname_converter is not None:
        colnames = [colname_converter[x].upper() if x in colname_converter else x for x in colnames]
    return fix_dup_names(colnames)


def file_row_names(raw_names, rowname_converter=None):
    """nabo/_io.py:416-427 on the first fields of the lines: quotes off, upper case, the converter, and the reference's OWN
    duplicate scheme for these: the first occurrence keeps its name, the n-th gets _n"""
    seen, out = {}, []
    for raw in raw_names:
        name = _clean(raw)
        if rowname_converter is not None and name in rowname_converter:
            name = rowname_converter[name].upper()
        if name not in seen:
            seen[name] = 1
        else:
            seen[name] += 1
            name = name + ("_%d" % seen[name])
        out.append(name)
    return out


def _open_bytes(fn):
    return gzip.open(fn, "rb") if fn.endswith(".gz") else open(fn, "rb")


class _Lines:
    """the first lines of a byte stream one at a time, then the rest as it comes"""

    def __init__(self, f):
        self.f, self.buf, self.eof = f, b"", False

    def _more(self):
        piece = self.f.read(READ_BYTES)
        if not piece:
            self.eof = True
        self.buf += piece

    def line(self):
        """the next line without its `\\n`, None at the end of the stream"""
        while b"\n" not in self.buf and not self.eof:
            self._more()
        if not self.buf:
            return None
        line, nl, self.buf = self.buf.partition(b"\n")
        return line

    def rest(self):
        while True:
            if self.buf:
                yield self.buf
                self.buf = b""
            if self.eof:
                return
            self._more()


def read_csv(source, sep=",", genes_in_columns=False, inv_log=None, value_dtype=float, null_thresh=None, rownames=None, colnames=None,
             colname_converter=None, rowname_converter=None, skip_lines=0, chunk_bytes=0, mem_budget=0, device=0):
    """Read a dense table of numbers into (matrix, genes, cells) on the MI355X: `matrix` has CountMatrix's attribute names
    (CsvMatrix.counts) with float64 or int64 values, `genes` and `cells` are the names as the reference's csv_to_h5 makes
    them.

    source: a file name (plain or `.gz`) or an object with read(n) that returns bytes; a gzipped file is inflated on the
    host and fed as it comes.  skip_lines lines are skipped; without `colnames` the next line is the header: split at sep,
    quotes off, upper case (a trailing `\\r` is taken off the last name: a departure).  Without `rownames` the first field
    of every line is the row's name (quotes off, upper case, rowname_converter, the n-th occurrence of a name gets _n) and
    the first column name is dropped; given `rownames` go through fix_dup_names and must be as many as the table has rows.
    Column names go through colname_converter and fix_dup_names.  null_thresh: values below it are 0; a field is an entry
    iff its value is not 0.  inv_log: the kept values become inv_log ** value on the host, as the reference computes them.
    Departures: `1_0` and digits outside ASCII, which numpy 1.26 accepts, are refused."""
    _, dtype = _kind(value_dtype)
    if hasattr(source, "read"):
        f, own = source, False
    else:
        f, own = _open_bytes(str(source)), True
    try:
        lines = _Lines(f)
        for _ in range(int(skip_lines)):
            if lines.line() is None:
                raise ValueError("ERROR: the file ends inside the %d lines to skip" % skip_lines)
        first_line = int(skip_lines)
        if colnames is None:
            head = lines.line()
            if head is None:
                raise ValueError("ERROR: the file has no header line")
            colnames, first_line = header_names(head, sep), first_line + 1
        col_names = column_names(colnames, rownames is not None, colname_converter)
        if not col_names:
            raise ValueError("ERROR: the table has no value column")
        with CsvReader(sep, len(col_names), rownames is None, dtype, null_thresh, first_line, chunk_bytes, mem_budget, device) as r:
            for piece in lines.rest():
                r.feed(piece)
            m = r.finish()
    finally:
        if own:
            f.close()
    if rownames is None:
        row_names = file_row_names(m.row_names, rowname_converter)
    else:
        row_names = fix_dup_names(rownames)
        if len(row_names) != m.n_rows:
            raise ValueError("ERROR: %d rownames were given, the table has %d rows" % (len(row_names), m.n_rows))
    if inv_log is not None:
        m.val = np.power(inv_log, m.val).astype(dtype)
        m.col_val = np.power(inv_log, m.col_val).astype(dtype)
    genes, cells = (col_names, row_names) if genes_in_columns else (row_names, col_names)
    return m.counts(genes_in_columns), genes, cells


def csv_to_h5(csv_fn, h5_fn, sep=",", genes_in_columns=False, inv_log=None, value_dtype=float, null_thresh=None, batch_size=500, rownames=None,
              colnames=None, colname_converter=None, rowname_converter=None, skip_lines=0):
    """The reference's csv_to_h5 (nabo/_io.py:238-287): a CSV table to a Nabo dataset file with names/{genes,cells},
    cell_data/<cell> and gene_data/<gene>, records of dtype [('idx', np.int64), ('val', value_dtype)] -- what the
    reference's np.rec.fromarrays of np.nonzero's indices gives.  The table is read by read_csv; batch_size is accepted and
    ignored (nothing is batched here).  An existing h5_fn is overwritten."""
    import h5py  # noqa: F401  (fail before the table is read, not after)
    _, dtype = _kind(value_dtype)
    m, genes, cells = read_csv(csv_fn, sep, genes_in_columns, inv_log, dtype, null_thresh, rownames, colnames, colname_converter, rowname_converter, skip_lines)
    if os.path.isfile(h5_fn):
        print("Overwriting %s" % h5_fn, flush=True)
        os.remove(h5_fn)
    write_dataset_file(h5_fn, m, genes, cells, dtype, idx_dtype=np.int64)
    return None
