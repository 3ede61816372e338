"""The CSV reader on the MI355X (include/nabo_csv.h), through CsvReader and read_csv, held byte for byte to the plain
restatement (tests/_csv_ref.py) and to what the reference wrote (tests/golden/csv.npz): both indexes, the values by their
bits, the row names and the counts of fields converted on the device and deferred to the host; the edges of the kernel's
geometry, built from nabo_csv_geometry; every split; the grammar's corners; one test per kind of error, each with a second,
later error in the file; and the file-level csv_to_h5.  Errors are compared by line and field, never by message text.

The kernels' grids are one workgroup per tile and no workgroup loops over tiles; the long-line case has lines of more than
three tiles (tiles without a `\\n`), the short-line case many lines per lane."""
import io
import json
import os
import re
import subprocess

import numpy as np
import pytest

import _csv_ref as cref
from test_csv_cpu import HARD, TABLES, golden_kwargs, reference_indexes, same_after_power, same_index
from test_mapping import _interpreter

HERE = os.path.dirname(os.path.abspath(__file__))
PRIMES = (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47, 53, 59, 61, 67, 71, 73, 79, 83, 89, 97, 101, 103, 107, 109, 113, 127, 131)


@pytest.fixture(scope="module")
def gold(golden):
    return golden("csv")


@pytest.fixture(scope="module")
def geo(gpu_lib):
    from nabo_amd import _csv
    return _csv.geometry()


def pieces(data, split):
    """the data fed whole (0), `split` bytes at a time, or in pieces of the primes in turn ("primes")"""
    if split == 0:
        return [data] if data else []
    out, at, k = [], 0, 0
    while at < len(data):
        n = PRIMES[k % len(PRIMES)] if split == "primes" else split
        out.append(data[at:at + n])
        at, k = at + n, k + 1
    return out


def run(body, sep=b",", n_cols=1, has_names=True, kind=0, thresh=None, first_line=0, chunk=0, split=0):
    """the body through the reader: ("ok", CsvMatrix, stats) or ("refused", line, field); after a refusal the handle must
    take nothing more"""
    from nabo_amd import _csv, _lib
    r = _csv.CsvReader(sep.decode("latin-1"), n_cols, has_names, int if kind else float, thresh, first_line, chunk)
    try:
        try:
            for piece in pieces(body, split):
                r.feed(piece)
            m = r.finish()
        except ValueError as e:
            hit = re.match(r"ERROR: line (\d+), field (\d+): ", str(e))
            assert hit, str(e)
            assert _lib.lib().nabo_csv_feed(r._h, b"1", 1) == _lib.E_INVALID and _lib.lib().nabo_csv_finish(r._h, None, None) == _lib.E_INVALID
            return "refused", int(hit.group(1)), int(hit.group(2))
        return "ok", m, r.stats()
    finally:
        r.close()


def agrees(body, chunk=0, split=0, **kw):
    """the library against the restatement on one body: the same bytes everywhere, or the same line and field"""
    got = run(body, chunk=chunk, split=split, **kw)
    try:
        p = cref.parse(body, **kw)
    except cref.Refused as e:
        assert got == ("refused", e.line, e.field), (got, str(e))
        return got
    assert got[0] == "ok", got
    m, stats = got[1], got[2]
    by_row, by_col = cref.indexes(p, kw.get("kind", 0))
    assert (m.n_rows, m.n_cols) == (p["n_rows"], p["n_cols"])
    assert same_index((m.row_ptr, m.col, m.val), by_row) and same_index((m.col_ptr, m.row, m.col_val), by_col)
    assert m.row_names == p["names"] and stats == p["stats"], (stats, p["stats"])
    return got


def table(rng, n_rows, n_cols, fmt, zeros=0.6, sep=b",", names=True, eol=b"\n"):
    v = rng.uniform(0, 1000, size=(n_rows, n_cols)) * (rng.random((n_rows, n_cols)) >= zeros)
    lines = [sep.join(([b"r%d" % i] if names else []) + [(fmt % x).encode() if x else b"0" for x in row]) for i, row in enumerate(v.tolist())]
    return eol.join(lines) + eol


# ---- the golden tables ----------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("s", ["A", "B", "C"])
def test_golden_equals_the_reference(gpu_lib, gold, s, tmp_path):
    kw, kind = golden_kwargs(gold, s)
    data = gold[s + "_csv"].tobytes()
    in_cols, inv_log = kw.get("genes_in_columns", False), kw.get("inv_log")
    args = dict(sep=kw.get("sep", ","), genes_in_columns=in_cols, value_dtype=int if kind else float, null_thresh=kw.get("null_thresh"), rownames=kw.get("rownames"))
    fn = str(tmp_path / "t.csv")
    with open(fn, "wb") as f:
        f.write(data)
    want = reference_indexes(gold, s, in_cols)
    for source in (fn, io.BytesIO(data)):
        m, genes, cells = gpu_lib.read_csv(source, inv_log=inv_log, chunk_bytes=4096, **args)
        rows, cols = ((m.cell_ptr, m.gene, m.val), (m.gene_ptr, m.cell, m.gene_val)) if in_cols else ((m.gene_ptr, m.cell, m.gene_val), (m.cell_ptr, m.gene, m.val))
        if inv_log is None:
            assert same_index(rows, want[0]) and same_index(cols, want[1])
        else:
            raw = reference_indexes(gold, s, in_cols, "raw")
            assert same_after_power(rows, raw[0], want[0], inv_log) and same_after_power(cols, raw[1], want[1], inv_log)
            plain = gpu_lib.read_csv(io.BytesIO(data), **args)[0]
            assert same_index((plain.cell_ptr, plain.gene, plain.val), raw[0]) and same_index((plain.gene_ptr, plain.cell, plain.gene_val), raw[1])
        assert genes == [str(x) for x in gold[s + "_genes"]] and cells == [str(x) for x in gold[s + "_cells"]]
        assert (m.n_genes, m.n_cells) == (60, 80)
    # the body against the restatement, statistics included: a file of 17-digit reprs is converted on the device
    body = data[data.index(b"\n") + 1:]
    got = agrees(body, sep=kw.get("sep", ",").encode(), n_cols=80 if not in_cols else 60, has_names="rownames" not in kw, kind=kind, thresh=kw.get("null_thresh"),
                 first_line=1, chunk=4096)
    assert got[2]["deferred"] == 0 and got[2]["converted"] == 4800


@pytest.mark.gpu
def test_gzip_and_header_rules(gpu_lib, gold, tmp_path):
    import gzip
    data = gold["A_csv"].tobytes()
    fn = str(tmp_path / "a.csv.gz")
    with gzip.open(fn, "wb") as f:
        f.write(b"# a comment\n# another\n" + data.replace(b"\n", b"\r\n"))
    m, genes, cells = gpu_lib.read_csv(fn, skip_lines=2, rowname_converter={"GENE3": "renamed"}, colname_converter={"CELL_A0": "first"})
    want = reference_indexes(gold, "A", False)
    assert same_index((m.gene_ptr, m.cell, m.gene_val), want[0]) and same_index((m.cell_ptr, m.gene, m.val), want[1])
    ref_genes, ref_cells = [str(x) for x in gold["A_genes"]], [str(x) for x in gold["A_cells"]]
    assert genes == ["RENAMED" if g == "GENE3" else g for g in ref_genes] and cells == ["FIRST"] + ref_cells[1:]      # (the \r is off the last name)
    with pytest.raises(ValueError) as e:
        gpu_lib.read_csv(io.BytesIO(b"# c\ng,a,b\nx,1,2\ny,1,z\n"), skip_lines=1)
    assert str(e.value).startswith("ERROR: line 4, field 3: ")
    with pytest.raises(ValueError):
        gpu_lib.read_csv(io.BytesIO(b"a,b\n1,2\n3,4\n"), rownames=["only one"])
    m, genes, cells = gpu_lib.read_csv(io.BytesIO(b"1,2\n0,4\n"), rownames=["x", "x"], colnames=["p", "q"], genes_in_columns=True, value_dtype=int, inv_log=2)
    assert (genes, cells) == (["P", "Q"], ["X_1", "X_2"]) and m.val.tolist() == [2, 4, 16] and m.val.dtype == np.int64


# ---- the geometry -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_long_lines(gpu_lib, geo):
    body = table(np.random.default_rng(1), 9, 6000, "%.6f", zeros=0.1)
    assert min(len(x) for x in body.split(b"\n")[:-1]) > 3 * geo["tile_bytes"]
    for chunk in (0, 40000):
        agrees(body, chunk=chunk, n_cols=6000)


@pytest.mark.gpu
def test_short_lines(gpu_lib, geo):
    body = table(np.random.default_rng(2), 700, 3, "%d", zeros=0.5, names=False)
    assert len(body) < geo["tile_bytes"] and body.count(b"\n") == 700
    for chunk in (0, 64):
        agrees(body, chunk=chunk, n_cols=3, has_names=False)


@pytest.mark.gpu
def test_fields_across_tiles(gpu_lib, geo):
    T, MN = geo["tile_bytes"], geo["max_name"]
    lines, size = [], 0
    while size < T - 150:
        lines.append(b"r%d,%d,0,%d.25\n" % (len(lines), len(lines) % 7, len(lines)))
        size += len(lines[-1])
    # a value whose first byte is the last byte of the tile: blanks in front of the value before it
    head = b"".join(lines)
    pad = T - 1 - len(head) - len(b"edge,") - len(b"7,")
    assert 0 < pad < geo["max_field"]
    body = head + b"edge," + b" " * pad + b"7,123456.789,3\n" + b"after,1,2,3\n"
    assert body[T - 1:T + 3] == b"1234" and body[T - 2:T - 1] == b","
    agrees(body, n_cols=3)
    # a name whose first byte is the last byte of the tile, and a line that ends exactly on the tile's end
    pad = T - 1 - len(head) - len(b"x,1,2,3\n")
    body = head + b"x,1," + b" " * pad + b"2,3\n" + b"name_across,4,5,6\nlast,7,8,9"
    assert body[T - 1:T + 4] == b"name_" and body[T - 2:T - 1] == b"\n"
    agrees(body, n_cols=3)
    agrees(body.replace(b"\n", b"\r\n"), n_cols=3)
    # the longest name, at the end of a tile, and one byte more
    ok = head + b"n" * MN + b",1,2,3\nz,4,5,6\n"
    assert agrees(ok, n_cols=3)[1].row_names[-2] == "n" * MN
    assert agrees(head + b"n" * (MN + 1) + b",1,2,3\nz,4,5,x\n", n_cols=3) == ("refused", len(lines) + 1, 1)
    for n_bytes in (T - 1, T, T + 1, 2 * T):                    # bodies that end around a tile's end
        body = b"a,1,0,3\n" * (n_bytes // 8 - 1) + b"b," + b"1" * (1 + n_bytes % 8) + b",0,3\n"
        assert len(body) == n_bytes
        agrees(body, n_cols=3)


@pytest.mark.gpu
def test_long_numbers(gpu_lib, geo):
    MF = geo["max_field"]
    digits = b"12345678901234567"
    at_limit = b"0" * (MF - len(digits) - 2) + digits + b".5"      # max_field bytes: the device converts it
    over = b"0" + at_limit                                          # one more: deferred, the same value
    assert len(at_limit) == MF and len(over) == MF + 1
    got = agrees(b"a,1," + at_limit + b",2\nb," + over + b",0,3\n", n_cols=3)
    assert got[2]["deferred"] == 1 and got[1].val[1] == got[1].val[3] == 12345678901234567.5
    # a long field that is zero, one that is the last of a line that is too short, and one that is no number
    got = agrees(b"a,1," + b"0" * (MF + 5) + b",2\n", n_cols=3)
    assert got[2] == dict(fields=3, entries=2, converted=2, deferred=1)
    assert agrees(b"a,1,2,3\nb,1," + b"0" * (MF + 5) + b"\nc,x,y,z\n", n_cols=3) == ("refused", 2, 4)
    assert agrees(b"a,1,2,3\nb,1," + b"0" * (MF + 5) + b"x,3\nc,x,y,z\n", n_cols=3) == ("refused", 2, 3)
    assert agrees(b"a,1,2,3\nb,1," + b"1" * 4097 + b",3\n", n_cols=3) == ("refused", 2, 3)
    # more than 19 digits, and the 17 - 19 digit halfway cases the device decides itself
    got = agrees(b"a,12345678901234567890,9007199254740993,1152921504606846977,1.00000000000000011102230246251565404236316680908203125\n", n_cols=4)
    assert got[2] == dict(fields=4, entries=4, converted=2, deferred=2)


@pytest.mark.gpu
def test_every_split_gives_the_same_bytes(gpu_lib, gold):
    data = gold["A_csv"].tobytes()
    body = data[data.index(b"\n") + 1:]
    first = None
    for chunk in (64, 4096, 0):
        for split in (0, "primes", 1):
            got = agrees(body, chunk=chunk, split=split, n_cols=80, first_line=1)
            m = got[1]
            blob = b"".join(x.tobytes() for x in (m.row_ptr, m.col, m.val, m.col_ptr, m.row, m.col_val)) + "\n".join(m.row_names).encode()
            first = first or blob
            assert blob == first, (chunk, split)


@pytest.mark.gpu
def test_line_ends(gpu_lib):
    rng = np.random.default_rng(4)
    body = table(rng, 40, 7, "%.3f")
    for chunk in (0, 64):
        for variant in (body.replace(b"\n", b"\r\n"), body[:-1], body[:-1] + b"\r", body + b"\n\n\n", body.replace(b"\n", b"\r\n") + b"\r\n\r\n", body + b"\n" * 200):
            got = agrees(variant, chunk=chunk, split=3 if chunk else 0, n_cols=7)
            assert got[1].n_rows == 40
    for body, kw, want in TABLES:
        agrees(body, **kw)
        agrees(body, chunk=64, split=1, **kw)


@pytest.mark.gpu
def test_zeros(gpu_lib, geo):
    v = np.arange(1, 31).reshape(5, 6)
    v[2, :] = 0
    v[:, 4] = 0
    body = b"".join(b"g%d," % i + b",".join(b"%d" % x for x in row) + b"\n" for i, row in enumerate(v.tolist()))
    m = agrees(body, n_cols=6)[1]
    assert np.diff(m.row_ptr).tolist() == [5, 5, 0, 5, 5] and np.diff(m.col_ptr).tolist() == [4, 4, 4, 4, 0, 4]
    got = agrees(b"g0,0,0.0,-0\ng1,0e5,.0,0.\n", n_cols=3)
    assert got[1].nnz == 0 and got[1].row_ptr.tolist() == [0, 0, 0] and got[1].col_ptr.tolist() == [0, 0, 0, 0]
    # nothing but `0,0,...`: 32 fields in every 64 bytes, and the same with ones: 32 ENTRIES in every 64 bytes
    n = geo["tile_bytes"] + 1000
    for digit in (b"0", b"1"):
        body = (b",".join([digit] * n) + b"\n") * 2
        got = agrees(body, n_cols=n, has_names=False)
        assert got[2]["fields"] == 2 * n and got[1].nnz == (0 if digit == b"0" else 2 * n)


@pytest.mark.gpu
def test_special_values(gpu_lib):
    got = agrees(b"x,nan,-inf,-0.0,1e-400,+Infinity,NaN,-nan\n", n_cols=7)
    assert got[1].col.tolist() == [0, 1, 4, 5, 6] and np.isnan(got[1].val[[0, 3, 4]]).all() and got[1].val[1] == -np.inf
    hard = [s for s in HARD if s.strip() == s][:40]
    assert len(hard) == 40
    for sep in (b",", b"\t"):
        got = agrees(b"row" + sep + sep.join(s.encode() for s in hard) + b"\n", sep=sep, n_cols=40)
        kept = [float(s) for s in hard if float(s) != 0]
        assert got[1].val.tobytes() == np.array(kept).tobytes() and got[2]["deferred"] > 0
    # null_thresh with a NaN present: a NaN is not below anything
    got = agrees(b"x,0.5,nan,2,-1,1.0\ny,-inf,inf,0.999,1e3,0\n", n_cols=5, thresh=1.0)
    assert got[1].col.tolist() == [1, 2, 4, 1, 3]


@pytest.mark.gpu
def test_int64_values(gpu_lib):
    body = b"a,5,-7,0,-0\nb,-9223372036854775808,9223372036854775807,1000000000000000000,999999999999999999\nc,+3,  4 ,0004,0\n"
    got = agrees(body, n_cols=4, kind=1)
    assert got[1].val.dtype == np.int64 and got[1].val.tolist() == [5, -7, -2 ** 63, 2 ** 63 - 1, 10 ** 18, 10 ** 18 - 1, 3, 4, 4]
    assert got[2] == dict(fields=12, entries=9, converted=9, deferred=3)
    got = agrees(body, n_cols=4, kind=1, thresh=4.5, chunk=64, split=1)
    assert got[1].val.tolist() == [5, 2 ** 63 - 1, 10 ** 18, 10 ** 18 - 1]
    assert agrees(b"a,1,2\nb,9223372036854775808,2\nc,x,1\n", n_cols=2, kind=1) == ("refused", 2, 2)


@pytest.mark.gpu
def test_other_separators(gpu_lib):
    rng = np.random.default_rng(6)
    for sep in (b"\t", b";", b" ", b"|"):
        agrees(table(rng, 30, 11, "%.4f", sep=sep), sep=sep, n_cols=11, chunk=64)
    from nabo_amd import _lib
    import ctypes as C
    h = C.c_void_p()
    assert _lib.lib().nabo_csv_create(99, 44, 3, 1, 0, 0, 0.0, 0, 0, C.byref(h)) == _lib.E_NODEVICE
    assert _lib.lib().nabo_csv_create(0, 44, 3, 1, 0, 0, 0.0, 0, 1000, C.byref(h)) == _lib.E_NOMEM      # a budget of 1000 bytes


# ---- errors: one per kind, each with a later one behind it ----------------------------------------------------------------
def error_body(geo, bad_line, later, kind):
    """2000 good lines of 4 values; line 120 replaced by bad_line, line 1600 (in another tile) by later"""
    if kind:
        lines = [b"r%d,%d,0,%d,%d" % (i, i, i % 9, i % 30) for i in range(2000)]
    else:
        lines = [b"r%d,%d.5,0,%d,1e%d" % (i, i, i % 9, i % 30) for i in range(2000)]
    lines[119], lines[1599] = bad_line, later
    assert len(b"\n".join(lines[:120])) < geo["tile_bytes"] < len(b"\n".join(lines[:1599]))
    return b"\n".join(lines) + b"\n"


ERRORS = [("too few fields", b"r,1,2,3", 5, 0), ("too many fields", b"r,1,2,3,4,5", 6, 0), ("an empty field", b"r,1,,3,4", 3, 0), ("a bad byte", b"r,1,2,3x,4", 4, 0),
          ("a float in int mode", b"r,1,2.5,3,4", 3, 1), ("an empty line in the middle", b"", 1, 0)]


@pytest.mark.gpu
@pytest.mark.parametrize("what,bad,field,kind", ERRORS, ids=[e[0] for e in ERRORS])
def test_the_lowest_error_wins(gpu_lib, geo, what, bad, field, kind):
    body = error_body(geo, bad, b"r,1,2", kind)
    for chunk, split in ((0, 0), (4096, 0), (64, 7)):
        assert agrees(body, chunk=chunk, split=split, n_cols=4, kind=kind, first_line=2) == ("refused", 2 + 120, field), (what, chunk)
    # the later error alone, and an earlier one of another kind in front of both
    alone = error_body(geo, b"r,1,2,3,4", b"r,1,2", kind)
    assert agrees(alone, n_cols=4, kind=kind) == ("refused", 1600, 4)
    assert agrees(b"r,x,2,3,4\n" + body, n_cols=4, kind=kind) == ("refused", 1, 2)


# ---- the file ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_file_level_csv_to_h5(gpu_lib):
    py = _interpreter()
    if py is None:
        pytest.skip("no interpreter with h5py in this image")
    r = subprocess.run([py, os.path.join(HERE, "_csv_case.py")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][len("RESULT "):])
    assert res["checked"] == 10 and res["differ"] == [], res
