"""The writer and the remap of include/nabo_counts.h in plain Python / numpy: the text as Python's `%d` writes it, line
by line; the remap entry by entry with dicts and sorted(); subsetting and merging on top of it, names and all.  Written
from the header's text, not from the library's code; the GPU tests hold the library to it byte for byte."""
import numpy as np

BANNER = b"%%MatrixMarket matrix coordinate integer general\n"


class Duplicate(Exception):
    """two kept columns of one row map to the same output column: the lowest (output row, output column)"""

    def __init__(self, row, col):
        Exception.__init__(self, "output row %d, output column %d" % (row, col))
        self.row, self.col = row, col


def mtx_text(n_genes, cell_ptr, gene, val, comments=b"", blank=False):
    """the whole text: banner, comments, size line, then cell by cell one line per entry; a cell without entries leaves a
    single newline when `blank` is set"""
    cell_ptr, gene, val = [np.asarray(x).tolist() for x in (cell_ptr, gene, val)]
    n_cells = len(cell_ptr) - 1
    out = [BANNER, comments, b"%d %d %d\n" % (n_genes, n_cells, len(gene))]
    for c in range(n_cells):
        if cell_ptr[c] == cell_ptr[c + 1] and blank:
            out.append(b"\n")
        out.extend(b"%d %d %d\n" % (gene[e] + 1, c + 1, val[e]) for e in range(cell_ptr[c], cell_ptr[c + 1]))
    return b"".join(out)


def index_of(lists, dtype):
    """(ptr, idx, val) of a list of lists of (index, value)"""
    ptr = np.zeros(len(lists) + 1, dtype=np.int64)
    np.cumsum([len(x) for x in lists], out=ptr[1:])
    flat = [p for x in lists for p in x]
    return ptr, np.array([p[0] for p in flat], dtype=np.int32), np.array([p[1] for p in flat], dtype=dtype)


def remap(ptr, idx, val, row_src, col_map, n_out_cols):
    """((out_ptr, out_idx, out_val), (csc_ptr, csc_idx, csc_val)), or Duplicate"""
    val = np.asarray(val)
    ptr, idx, vals = np.asarray(ptr).tolist(), np.asarray(idx).tolist(), val.tolist()
    col_map = np.asarray(col_map).tolist()
    rows, cols, dup = [], [[] for _ in range(n_out_cols)], None
    for r, s in enumerate(np.asarray(row_src).tolist()):
        kept = sorted((col_map[idx[e]], e) for e in range(ptr[s], ptr[s + 1]) if col_map[idx[e]] >= 0)
        for a, b in zip(kept, kept[1:]):
            if a[0] == b[0] and dup is None:
                dup = (r, a[0])
        rows.append([(c, e) for c, e in kept])
        for c, e in kept:
            cols[c].append((r, e))
    if dup is not None:
        raise Duplicate(*dup)
    # values by position, so that a float32 payload keeps its bits
    def build(lists):
        p, i, e = index_of(lists, np.int64)
        return p, i, val[e] if len(e) else np.zeros(0, dtype=val.dtype)
    return build(rows), build(cols)


def subset(ptr, idx, val, n_genes, rows):
    return remap(ptr, idx, val, rows, list(range(n_genes)), n_genes)


def merge(matrices, gene_names, cell_names, suffixes, cell_order):
    """matrices: (cell_ptr, gene, val) each.  (csr, csc, genes, cells) with the genes the sorted union, the cells
    `name-suffix` in cell_order, records ascending by index"""
    genes = sorted(set(g for names in gene_names for g in names))
    where = {g: n for n, g in enumerate(genes)}
    cell_of = {}
    for k, (ptr, idx, val) in enumerate(matrices):
        ptr, idx, val = [np.asarray(x).tolist() for x in (ptr, idx, val)]
        for c, name in enumerate(cell_names[k]):
            cell_of[name + "-" + suffixes[k]] = sorted((where[gene_names[k][idx[e]]], val[e]) for e in range(ptr[c], ptr[c + 1]))
    rows = [cell_of[c] for c in cell_order]
    cols = [[] for _ in genes]
    for r, row in enumerate(rows):
        for g, v in row:
            cols[g].append((r, v))
    return index_of(rows, np.uint32), index_of(cols, np.uint32), genes, list(cell_order)


def write_dataset(fn, genes, cells, csr, csc, value_dtype=np.int64):
    """a Nabo dataset file with h5py, straight from the two indexes: EVERY cell and gene gets a dataset (the reference's own
    h5_to_mtx fails on a cell without one)"""
    import h5py
    dtype = [("idx", np.uint), ("val", value_dtype)]
    with h5py.File(fn, "w") as h5:
        grp = h5.create_group("names")
        grp.create_dataset("genes", chunks=None, data=[x.encode("ascii") for x in genes])
        grp.create_dataset("cells", chunks=None, data=[x.encode("ascii") for x in cells])
        for group, names, (ptr, idx, val) in (("cell_data", cells, csr), ("gene_data", genes, csc)):
            rec = np.zeros(len(idx), dtype=dtype)
            rec["idx"], rec["val"] = idx, val
            grp = h5.create_group(group)
            for i, name in enumerate(names):
                grp.create_dataset(name, data=rec[ptr[i]:ptr[i + 1]], chunks=None)


def read_records(fn, group, names):
    """(lengths, idx, val) of the datasets `names` of a group, concatenated, as int64"""
    import h5py
    with h5py.File(fn, "r") as h5:
        recs = [h5[group][n][:] for n in names]
    cat = lambda k: np.concatenate([r[k] for r in recs] + [np.zeros(0, np.int64)]).astype(np.int64)  # noqa: E731
    return np.array([len(r) for r in recs], dtype=np.int64), cat("idx"), cat("val")


def sorted_records(lens, idx, val):
    """the records of read_records with every dataset sorted by idx (stable)"""
    idx, val, at = idx.copy(), val.copy(), 0
    for n in lens.tolist():
        o = np.argsort(idx[at:at + n], kind="stable")
        idx[at:at + n], val[at:at + n] = idx[at:at + n][o], val[at:at + n][o]
        at += n
    return lens, idx, val
