"""The Matrix Market reader of include/nabo_ingest.h in plain Python: the grammar from bytes to either triplets or
(status, line), the two numpy stable sorts that make the cell and the gene index of them, and fix_dup_names.  Written
from the header's text, not from the library's code; the GPU tests hold the library to it byte for byte."""
import numpy as np

E_INVALID, E_UNSUPPORTED = -1, -5
LONG, SYNTAX, REAL, FIELDS, GENE, CELL, VALUE, EXCESS, FEW, DUP = 1, 2, 3, 4, 5, 6, 7, 8, 9, 10
BLANKS = b" \t"


class Refused(Exception):
    def __init__(self, status, line, code=None):
        Exception.__init__(self, "status %d at line %s (code %s)" % (status, line, code))
        self.status, self.line, self.code = status, line, code


def _unsigned(word):
    """the value of a run of digits, None when it is none; 10**19 stands for 'more than 19 digits after the zeros'"""
    if not word or not all(48 <= b <= 57 for b in word):
        return None
    digits = word.lstrip(b"0")
    return 10 ** 19 if len(digits) > 19 else int(digits or b"0")


def parse_header(data):
    """(n_genes, n_cells, nnz, number of header lines, offset of the body)"""
    pos, n, banner = 0, 0, False
    while True:
        if pos >= len(data):
            raise Refused(E_INVALID, n + 1)
        end = data.find(b"\n", pos)
        line, nxt = (data[pos:], len(data)) if end < 0 else (data[pos:end], end + 1)
        if line.endswith(b"\r"):
            line = line[:-1]
        if not banner:
            words = line[14:].replace(b"\t", b" ").split()
            if (not line.startswith(b"%%MatrixMarket") or len(words) != 4 or [w.lower() for w in words[:2]] != [b"matrix", b"coordinate"]
                    or words[2].lower() not in (b"integer", b"real") or words[3].lower() != b"general"):
                raise Refused(E_INVALID, n + 1)
            banner = True
        elif not line.startswith(b"%"):
            v = [_unsigned(w) for w in line.replace(b"\t", b" ").split(b" ") if w]
            if len(v) != 3 or None in v:
                raise Refused(E_INVALID, n + 1)
            if v[0] >= 2 ** 31 or v[1] >= 2 ** 31 or v[2] >= 2 ** 32 - 1:
                raise Refused(E_UNSUPPORTED, n + 1)
            return v[0], v[1], v[2], n + 1, nxt
        n, pos = n + 1, nxt


def parse_line(line, n_genes, n_cells, max_line):
    """(gene, cell, value) 1-based, None for a skipped line, or the code of what is wrong"""
    if len(line) > max_line:
        return LONG
    if line.endswith(b"\r"):
        line = line[:-1] + b" "
    body = line.strip(BLANKS)
    if not body or body[:1] == b"%":
        return None
    # the first offending byte from the left; a fourth field offends at its first digit
    fields, indig = 0, False
    for i, b in enumerate(line):
        if b in BLANKS:
            fields, indig = fields + indig, False
        elif 48 <= b <= 57:
            if not indig and fields == 3:
                return FIELDS
            indig = True
        else:
            return REAL if b == 46 or (b in b"eE" and indig) else SYNTAX
    v = [_unsigned(w) for w in body.replace(b"\t", b" ").split(b" ") if w]
    if len(v) != 3:
        return FIELDS
    if not 1 <= v[0] <= n_genes:
        return GENE
    if not 1 <= v[1] <= n_cells:
        return CELL
    if v[2] > 2 ** 32 - 1:
        return VALUE
    return tuple(v)


def parse(data, max_line):
    """the whole file: (n_genes, n_cells, gene, cell, val) with 0-based int64 indices in FILE order, or Refused with the
    status and the 1-based line (None for a duplicate, which has no single line)"""
    n_genes, n_cells, nnz, n_head, pos = parse_header(bytes(data))
    body = bytes(data)[pos:]
    lines = body.split(b"\n")
    if lines[-1] == b"":
        lines.pop()
    out = []
    for k, line in enumerate(lines):
        r = parse_line(line, n_genes, n_cells, max_line)
        if r is None:
            continue
        if not isinstance(r, tuple):
            raise Refused(E_INVALID, n_head + k + 1, r)
        out.append(r)
        if len(out) > nnz:
            raise Refused(E_INVALID, n_head + k + 1, EXCESS)
    if len(out) != nnz:
        raise Refused(E_INVALID, n_head + len(lines), FEW)
    t = np.array(out, dtype=np.int64).reshape(-1, 3)
    gene, cell, val = t[:, 0] - 1, t[:, 1] - 1, t[:, 2]
    if len(np.unique(cell * 2 ** 31 + gene)) != nnz:
        raise Refused(E_INVALID, None, DUP)
    return n_genes, n_cells, gene, cell, val


def index_by(major, minor, val, n_major):
    """(ptr int64 [n_major + 1], minor int32, val uint32) ordered by (major, minor): two stable sorts"""
    o = np.argsort(minor, kind="stable")
    o = o[np.argsort(major[o], kind="stable")]
    ptr = np.zeros(n_major + 1, dtype=np.int64)
    np.cumsum(np.bincount(major, minlength=n_major), out=ptr[1:])
    return ptr, minor[o].astype(np.int32), val[o].astype(np.uint32)


def csr_csc(parsed):
    n_genes, n_cells, gene, cell, val = parsed
    return index_by(cell, gene, val, n_cells), index_by(gene, cell, val, n_genes)


def transpose(ptr, idx, val, n_cols):
    """CSR -> CSC by one stable argsort of the column indices"""
    ptr, idx, val = np.asarray(ptr, dtype=np.int64), np.asarray(idx, dtype=np.int64), np.asarray(val, dtype=np.float32)
    rows = np.repeat(np.arange(len(ptr) - 1, dtype=np.int64), np.diff(ptr))
    o = np.argsort(idx, kind="stable")
    out_ptr = np.zeros(n_cols + 1, dtype=np.int64)
    np.cumsum(np.bincount(idx, minlength=n_cols), out=out_ptr[1:])
    return out_ptr, rows[o].astype(np.int32), val[o]


def fix_dup_names(names):
    """upper case; a name that then occurs more than once gets _1, _2, ... in order of appearance"""
    upper = [str(x).upper() for x in names]
    count = {}
    for x in upper:
        count[x] = count.get(x, 0) + 1
    seen, out = {}, []
    for x in upper:
        if count[x] > 1:
            seen[x] = seen.get(x, 0) + 1
            x = "%s_%d" % (x, seen[x])
        out.append(x)
    return out


def second_column(data):
    """the gene names of a genes.tsv / features.tsv: the second whitespace-separated field of every line"""
    return [line.split()[1].decode("UTF-8") for line in bytes(data).splitlines() if line.strip()]


def barcodes(data):
    return [line.decode("UTF-8").upper() for line in bytes(data).split(b"\n") if line != b""]


def mtx_text(n_genes, n_cells, gene, cell, val, comments=(b"%",)):
    """10x-shaped text of 0-based triplets, in the order given"""
    head = b"%%MatrixMarket matrix coordinate integer general\n" + b"".join(c + b"\n" for c in comments)
    body = b"".join(b"%d %d %d\n" % (g + 1, c + 1, v) for g, c, v in zip(gene.tolist(), cell.tolist(), val.tolist()))
    return head + b"%d %d %d\n" % (n_genes, n_cells, len(gene)) + body
