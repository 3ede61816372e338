"""The CSV reader of include/nabo_csv.h in plain Python: the grammar from bytes to either entries or (line, field, code),
the entry rule, the two indexes, the name rules of the reference's csv_to_h5, and -- with Python ints -- the device's
decimal -> double rule INCLUDING its verdict (converted on the device, or deferred to the host).  Written from the header's
text, not from the library's code; the GPU tests hold the library to it byte for byte."""
import re
import struct

import numpy as np

E_INVALID = -1
VALUE, DEFER = 0, -1
EMPTY_LINE, TOO_MANY, EMPTY, BAD, FLOAT, RANGE, NAME_LONG, FIELD_LONG, TOO_FEW = 1, 2, 3, 4, 5, 6, 7, 8, 9
MAX_FIELD, MAX_NAME, HARD_FIELD = 256, 1024, 4096
Q_MIN, Q_MAX = -342, 308
M64 = 2 ** 64 - 1
INF_BITS, NAN_BITS, SIGN = 0x7FF0000000000000, 0x7FF8000000000000, 1 << 63

NUMBER = re.compile(rb"([+-]?)(?:([0-9]+)(\.([0-9]*))?|\.([0-9]+))(?:[eE]([+-]?[0-9]+))?\Z")
SPECIAL = re.compile(rb"([+-]?)(inf|infinity|nan)\Z", re.I)


class Refused(Exception):
    def __init__(self, line, field, code):
        Exception.__init__(self, "line %d, field %d (code %d)" % (line, field, code))
        self.status, self.line, self.field, self.code = E_INVALID, line, field, code


def pow5_table():
    """{q: the 128-bit power of five for q}: 5^q with its highest bit at bit 127 and the rest cut off (q >= 0); an upper
    bound of 2^b / 5^-q cut down to 128 bits (q < 0)"""
    out = {}
    for q in range(Q_MIN, 0):
        p = 5 ** -q
        z = p.bit_length()
        c = 2 ** (z + 127 if q >= -27 else 2 * z + 128) // p + 1
        out[q] = c >> (c.bit_length() - 128)
    for q in range(0, Q_MAX + 1):
        p = 5 ** q
        out[q] = p << (128 - p.bit_length()) if p.bit_length() <= 128 else p >> (p.bit_length() - 128)
    return out


POW5 = pow5_table()


def bits_of(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def decimal_to_double(w, q):
    """w * 10^q, w below 10^19: (VALUE, bits without sign) when the device's rule proves the rounding, (DEFER, None)"""
    if w == 0 or q < Q_MIN:
        return VALUE, 0
    if q > Q_MAX:
        return VALUE, INF_BITS
    if w <= 2 ** 53 and -22 <= q <= 22:
        return VALUE, bits_of(float(w) / float(10 ** -q) if q < 0 else float(w) * float(10 ** q))
    lz = 64 - w.bit_length()
    w <<= lz
    t_hi, t_lo = POW5[q] >> 64, POW5[q] & M64
    hi, lo = (w * t_hi) >> 64, (w * t_hi) & M64
    if hi & 0x1FF == 0x1FF:
        lo += (w * t_lo) >> 64
        if lo > M64:
            lo, hi = lo & M64, hi + 1
    if lo == M64 and not -27 <= q <= 55:
        return DEFER, None
    upper = hi >> 63
    m = hi >> (upper + 9)
    p2 = ((217706 * q) >> 16) + 63 + upper - lz + 1023
    if p2 <= 0:
        if -p2 + 1 >= 64:
            return VALUE, 0
        m >>= -p2 + 1
        m = (m + (m & 1)) >> 1
        return VALUE, m
    if lo <= 1 and -4 <= q <= 23 and m & 3 == 1 and (m << (upper + 9)) == hi:
        m &= ~1
    m = (m + (m & 1)) >> 1
    if m >= 2 << 52:
        m, p2 = 1 << 52, p2 + 1
    m &= ~(1 << 52)
    if p2 >= 0x7FF:
        return VALUE, INF_BITS
    return VALUE, p2 << 52 | m


def strip_field(f, line_end):
    if line_end and f.endswith(b"\r"):
        f = f[:-1]
    return f.strip(b" \t")


def convert(f, line_end, kind):
    """one value field: (VALUE, bits) converted on the device, (DEFER, bits) with the bits the host's strtod / strtoll gives,
    or (error code, None)"""
    body = strip_field(f, line_end)
    if not body:
        return EMPTY, None
    sp, num = SPECIAL.match(body), NUMBER.match(body)
    if not sp and not num:
        return BAD, None
    if kind == 1:
        if sp or num.group(3) is not None or num.group(5) is not None or num.group(6) is not None:
            return FLOAT, None
        v = int(body)
        if len(num.group(2).lstrip(b"0")) > 18 or len(f) > MAX_FIELD:
            return (DEFER, v & M64) if -2 ** 63 <= v < 2 ** 63 else (RANGE, None)
        return VALUE, v & M64
    sign = SIGN if body[:1] == b"-" else 0
    if sp:
        code, bits = VALUE, sign | (NAN_BITS if sp.group(2).lower() == b"nan" else INF_BITS)
    else:
        ints, frac = num.group(2) or b"", (num.group(4) if num.group(2) is not None else num.group(5)) or b""
        sig = (ints + frac).lstrip(b"0")
        if len(sig) > 19:
            code, bits = DEFER, None
        else:
            code, bits = decimal_to_double(int(sig or b"0"), int(num.group(6) or b"0") - len(frac))
            bits = None if bits is None else bits | sign
    if len(f) > MAX_FIELD:
        code = DEFER
    if code == DEFER:
        bits = bits_of(float(body)) if not sp else bits
    return code, bits


def keeps(kind, bits, thresh):
    """the entry rule: below the threshold the value is 0 (a NaN is not below anything); kept iff it is not 0"""
    v = float(bits - 2 ** 64 if bits >> 63 else bits) if kind == 1 else struct.unpack("<d", struct.pack("<Q", bits))[0]
    if v == 0:
        return False
    return not (thresh is not None and v < thresh)


def parse(data, sep=b",", n_cols=1, has_names=True, kind=0, thresh=None, first_line=0):
    """the body of a table: a dict with n_rows, the entries in file order (row, col int64; bits uint64), the raw names and
    the statistics -- or Refused with the lowest (line, field)"""
    lines = bytes(data).split(b"\n")
    if lines[-1] == b"":
        lines.pop()
    while lines and lines[-1] in (b"", b"\r"):
        lines.pop()
    n_fields = n_cols + bool(has_names)
    rows, cols, bits, names = [], [], [], []
    stats = dict(fields=0, entries=0, converted=0, deferred=0)
    for k, line in enumerate(lines):
        no = first_line + k + 1
        if line in (b"", b"\r"):
            raise Refused(no, 1, EMPTY_LINE)
        fields = line.split(sep)
        for i, f in enumerate(fields):
            if i >= n_fields:
                raise Refused(no, i + 1, TOO_MANY)
            last = i == len(fields) - 1
            if has_names and i == 0:
                if len(f) > MAX_NAME:
                    raise Refused(no, 1, NAME_LONG)
                names.append(f)
                continue
            if len(f) > HARD_FIELD:
                raise Refused(no, i + 1, FIELD_LONG)
            code, b = convert(f, last, kind)
            if code > 0:
                raise Refused(no, i + 1, code)
            stats["fields"] += 1
            stats["converted" if code == VALUE else "deferred"] += 1
            if keeps(kind, b, thresh):
                rows.append(k), cols.append(i - bool(has_names)), bits.append(b)
        if len(fields) < n_fields:
            raise Refused(no, len(fields) + 1, TOO_FEW)
    stats["entries"] = len(bits)
    return dict(n_rows=len(lines), n_cols=n_cols, row=np.array(rows, dtype=np.int64), col=np.array(cols, dtype=np.int64),
                bits=np.array(bits, dtype=np.uint64), names=[x.decode("latin-1") for x in names] if has_names else None, stats=stats)


def indexes(p, kind=0):
    """((row_ptr, col int32, val), (col_ptr, row int32, val)) of a parsed table; val float64 or int64 by bits"""
    dt = np.int64 if kind == 1 else np.float64
    val = p["bits"].view(dt)
    row_ptr, col_ptr = np.zeros(p["n_rows"] + 1, np.int64), np.zeros(p["n_cols"] + 1, np.int64)
    np.cumsum(np.bincount(p["row"], minlength=p["n_rows"]), out=row_ptr[1:])
    np.cumsum(np.bincount(p["col"], minlength=p["n_cols"]), out=col_ptr[1:])
    o = np.argsort(p["col"], kind="stable")
    return (row_ptr, p["col"].astype(np.int32), val), (col_ptr, p["row"][o].astype(np.int32), val[o])


# ---- the names, by the reference's rules (nabo/_io.py:345-369, :416-427) ------------------------------------------------
def clean(name):
    return name.strip('"').strip("'").upper()


def fix_dup_names(names):
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


def header_names(line, sep):
    text = line.decode("latin-1")
    return [clean(x) for x in (text[:-1] if text.endswith("\r") else text).split(sep)]


def column_names(colnames, rownames_given, converter=None):
    colnames = list(colnames) if rownames_given else list(colnames)[1:]
    if converter is not None:
        colnames = [converter[x].upper() if x in converter else x for x in colnames]
    return fix_dup_names(colnames)


def file_row_names(raw, converter=None):
    seen, out = {}, []
    for name in raw:
        name = clean(name)
        if converter is not None and name in converter:
            name = converter[name].upper()
        seen[name] = seen.get(name, 0) + 1
        out.append(name if seen[name] == 1 else "%s_%d" % (name, seen[name]))
    return out


def read_table(data, sep=",", genes_in_columns=False, inv_log=None, kind=0, thresh=None, rownames=None, colnames=None, colname_converter=None,
               rowname_converter=None, skip_lines=0):
    """the whole file as csv_to_h5 reads it: (by-row index, by-column index, row names, column names); the values after
    inv_log"""
    data = bytes(data)
    pos = 0
    for _ in range(skip_lines):
        pos = data.index(b"\n", pos) + 1
    first = skip_lines
    if colnames is None:
        end = data.index(b"\n", pos)
        colnames, pos, first = header_names(data[pos:end], sep), end + 1, first + 1
    cols = column_names(colnames, rownames is not None, colname_converter)
    p = parse(data[pos:], sep.encode("latin-1"), len(cols), rownames is None, kind, thresh, first)
    rows = file_row_names(p["names"], rowname_converter) if rownames is None else fix_dup_names(rownames)
    by_row, by_col = indexes(p, kind)
    if inv_log is not None:
        by_row = by_row[:2] + (np.power(inv_log, by_row[2]).astype(by_row[2].dtype),)
        by_col = by_col[:2] + (np.power(inv_log, by_col[2]).astype(by_col[2].dtype),)
    return by_row, by_col, rows, cols
