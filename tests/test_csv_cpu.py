"""The CSV reader (include/nabo_csv.h, nabo_amd/_csv.py) without a GPU: the plain restatement (tests/_csv_ref.py) against
Python's float() on the hard strings and on 10^5 seeded ones, its table of powers of five against Python ints, the
restatement against what the reference wrote (tests/golden/csv.npz, tools/gen_golden_csv.py) and against cases written by
hand, the name rules, the header's symbols, the argument checks, the no-device failure -- and the host half of the reader
with the number routine the kernel shares (nabo_amd/csrc/csv_host.h, csv_number.h) built with a small main under the
address and undefined-behaviour sanitizers as a program of its own, held to the restatement field by field."""
import ctypes as C
import io
import json
import os
import random
import re
import struct
import subprocess

import numpy as np
import pytest

import nabo_amd
from nabo_amd import _csv, _lib

import _csv_ref as cref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the strings the issue names, then the edges of the rule: q at +-22 / +-23, w at 2^53 and 2^53 + 1, halfway cases
HARD = ["9007199254740993", "1e23", "8.41e21", "2.2250738585072011e-308", "1.7976931348623158e308", "1.7976931348623159e308", "4.9e-324",
        "2.4703282292062327e-324", "2e-324", "0.1", "123456789012345678e-20",
        "9007199254740992", "9007199254740992e22", "9007199254740992e23", "9007199254740992e-22", "9007199254740992e-23", "9007199254740993e22",
        "9007199254740993e-22", "1e22", "1e-22", "1e-23", "3e23", "7e-23",
        "9007199254740993.0", "18014398509481985", "1152921504606846977", "9223372036854775809",            # halfway, 16 - 19 digits
        "9007199254740993.00000000000", "90071992547409930000000e-7", "1.00000000000000011102230246251565404236316680908203125",
        "1.00000000000000011102230246251565404236316680908203124", "1.00000000000000011102230246251565404236316680908203126",   # and more than 19
        "0", "-0.0", "+0", "0e999999", "1e-400", "1e400", "-1e400", "1e309", "1e308", "5e-324", "3e-324", "2.4703282292062328e-324",
        "4.9406564584124654e-324", "2.2250738585072014e-308", "2.2250738585072009e-308", "1.7976931348623157e308",
        "123456789012345678901234567890", "0.000000000000000000000000000001", "1.", ".5", "+.5e-3", "00012.5000", "1E5", "1e+5", "12345678901234567890e-19",
        "inf", "-inf", "+Infinity", "iNf", "nan", "-nan", "NaN", "  12.5\t", "6.02214076e23", "6.62607015e-34", "1e55", "1e56", "1e-27", "1e-28",
        "9999999999999999999", "9999999999999999999e-342", "1844674407370955161e-324", "7.3177701707893310e+15", "5e-325"]
REFUSED = ["", " ", "\t", "1e", "e5", ".", "-", "+", "--1", "1-", "1 2", "NA", "na", "null", '"1"', "'1'", "0x10", "1_0", "1e5.0", "1.2.3", "infin", "nanx",
           "1,5", "١".encode().decode("latin-1"), "1e+", "+-1", "1d5", "1f", "1L", "Infinity8"]


def seeded_strings():
    """at least 10^5 strings: repr of random doubles, of doubles with uniform exponents, their low digits moved by +-1, and
    %.3f, %d and %e forms"""
    rng = random.Random(20250305)
    out = []
    for _ in range(40000):
        x = struct.unpack("<d", struct.pack("<Q", rng.getrandbits(64)))[0]
        if x == x and abs(x) != float("inf"):
            out.append(repr(x))
    for _ in range(30000):
        out.append(repr(rng.uniform(1, 10) * 10.0 ** rng.randint(-330, 308)))
    for s in out[:20000]:
        m = re.match(r"(-?)(\d)\.?(\d*)(e[+-]\d+)?$", s.replace("e-0", "e-").replace("e+0", "e+"))
        if m and m.group(3):
            digits = m.group(2) + m.group(3)
            moved = str(int(digits) + rng.choice((-1, 1))).rjust(len(digits), "0")
            out.append("%s%s.%s%s" % (m.group(1), moved[:len(moved) - len(m.group(3))], moved[len(moved) - len(m.group(3)):], m.group(4) or ""))
    for _ in range(10000):
        out += ["%.3f" % rng.uniform(0, 1000), "%d" % rng.randrange(0, 10 ** rng.randrange(1, 22)), "%e" % rng.uniform(0, 1e10), "%d" % rng.randrange(0, 60)]
    assert len(out) >= 100000
    return out


@pytest.fixture(scope="module")
def strings():
    return HARD + seeded_strings()


@pytest.fixture(scope="module")
def gold(golden):
    return golden("csv")


def test_restatement_equals_python_float(strings):
    n_value = n_defer = 0
    for s in strings:
        code, bits = cref.convert(s.encode(), False, 0)
        assert code in (cref.VALUE, cref.DEFER), s
        assert struct.pack("<Q", bits) == struct.pack("<d", float(s)), s
        n_value, n_defer = n_value + (code == cref.VALUE), n_defer + (code == cref.DEFER)
    assert n_value > 95000 and n_defer > 100                    # the long %d forms and the long halfway cases are the host's
    want = {"9007199254740993": 0x4340000000000000, "1e23": 0x44B52D02C7E14AF6, "1.7976931348623159e308": cref.INF_BITS, "2e-324": 0, "4.9e-324": 1,
            "2.4703282292062327e-324": 0, "2.4703282292062328e-324": 1, "0.1": 0x3FB999999999999A, "-0.0": cref.SIGN, "1e-400": 0, "-nan": cref.SIGN | cref.NAN_BITS}
    for s, bits in want.items():
        assert cref.convert(s.encode(), False, 0)[1] == bits, s
    # every string of 19 digits or fewer in HARD is decided by the rule itself; the longer ones are deferred
    for s in HARD:
        sig = re.sub(r"[eE].*", "", s.strip()).replace(".", "").lstrip("+-").lstrip("0")
        if sig.isdigit() or sig == "":
            assert (cref.convert(s.encode(), False, 0)[0] == cref.DEFER) == (len(sig) > 19), s
    for s in REFUSED:
        assert cref.convert(s.encode("latin-1"), False, 0)[0] > 0, s
    assert cref.convert(b"", False, 0)[0] == cref.EMPTY and cref.convert(b" \t", False, 0)[0] == cref.EMPTY and cref.convert(b"x", False, 0)[0] == cref.BAD
    assert cref.convert(b"1.5\r", True, 0)[0] == cref.VALUE and cref.convert(b"1.5\r", False, 0)[0] == cref.BAD


def test_restatement_int64_fields():
    for s, want in (("0", 0), ("-0", 0), ("+17", 17), ("  42 ", 42), ("000123", 123), ("999999999999999999", 10 ** 18 - 1), ("-999999999999999999", 1 - 10 ** 18)):
        assert cref.convert(s.encode(), False, 1) == (cref.VALUE, want & cref.M64), s
    for s, want in (("1000000000000000000", 10 ** 18), ("9223372036854775807", 2 ** 63 - 1), ("-9223372036854775808", -2 ** 63),
                    ("0000000000000000000000000000000000001", 1)):
        code, bits = cref.convert(s.encode(), False, 1)
        assert bits == want & cref.M64 and code == (cref.DEFER if len(s.lstrip("+-0")) > 18 else cref.VALUE), s
    assert cref.convert(b"9223372036854775808", False, 1)[0] == cref.RANGE and cref.convert(b"-9223372036854775809", False, 1)[0] == cref.RANGE
    for s in ("1.0", "1e3", ".5", "1.", "inf", "nan"):
        assert cref.convert(s.encode(), False, 1)[0] == cref.FLOAT, s
    for s in ("", "x", "1_0", "0x1", "--1"):
        assert cref.convert(s.encode(), False, 1)[0] in (cref.EMPTY, cref.BAD), s


def test_powers_of_five_against_python_ints():
    t = cref.POW5
    assert sorted(t) == list(range(-342, 309)) and all(2 ** 127 <= v < 2 ** 128 for v in t.values())
    for q in range(0, 309):                                     # 5^q cut to 128 bits: floor
        e = (5 ** q).bit_length() - 128
        assert t[q] * 2 ** e <= 5 ** q < (t[q] + 1) * 2 ** e if e >= 0 else t[q] == 5 ** q << -e
    for q in range(-342, 0):                                    # the reciprocal: an upper bound, tight to one unit
        p = 5 ** -q
        b = 127 + p.bit_length()
        assert (t[q] - 1) * p <= 2 ** b < t[q] * p or q < -27
        assert (t[q] - 1) * p <= 2 ** b <= (t[q] + 1) * p
    assert t[0] == 1 << 127 and t[1] == 5 << 125 and t[-1] == (2 ** 130 // 5 + 1)


def reference_indexes(d, s, in_cols, which="val"):
    """((row_ptr, col, val), (col_ptr, row, val)) from the records the reference wrote; which="raw": from its run without
    inv_log"""
    def one(group):
        ptr = np.zeros(d[s + "_%s_len" % group].shape[0] + 1, np.int64)
        np.cumsum(d[s + "_%s_len" % group], out=ptr[1:])
        return ptr, d[s + "_%s_idx" % group].astype(np.int32), d[s + "_%s_%s" % (group, which)]
    return (one("cell"), one("gene")) if in_cols else (one("gene"), one("cell"))


def same_index(a, b):
    return all(x.dtype == y.dtype and x.tobytes() == y.tobytes() for x, y in zip(a, b))


# `inv_log ** val` is numpy's power.  It is not correctly rounded: the build that wrote the golden records (1.26.4, SIMD)
# and the build in use are each within 1 ulp of the exact power, so they are within 2 ulps of each other -- and equal to
# neither in general.  What IS exact: the values in front of the power (the parser's), and the power of the numpy in use.
POWER_ULPS = 2


def same_after_power(got, want_raw, want_val, inv_log):
    """an index after inv_log against the reference's: pointers and indices equal, the values the power of the reference's
    raw values by the numpy in use, and within POWER_ULPS of what the reference's numpy wrote"""
    ok = same_index(got[:2], want_raw[:2]) and got[2].tobytes() == np.power(inv_log, want_raw[2]).tobytes()
    return ok and int(np.abs(got[2].view(np.int64) - want_val[2].view(np.int64)).max()) <= POWER_ULPS


def golden_kwargs(d, s):
    kw = json.loads(str(d["meta"]))[s]["kwargs"]
    return kw, 1 if kw.get("value_dtype") == "int" else 0


@pytest.mark.parametrize("s", ["A", "B", "C"])
def test_restatement_reproduces_the_reference(gold, s):
    kw, kind = golden_kwargs(gold, s)
    data = gold[s + "_csv"].tobytes()
    by_row, by_col, rows, cols = cref.read_table(data, kw.get("sep", ","), kw.get("genes_in_columns", False), kw.get("inv_log"), kind, kw.get("null_thresh"),
                                                 kw.get("rownames"))
    in_cols = kw.get("genes_in_columns", False)
    want = reference_indexes(gold, s, in_cols)
    if kw.get("inv_log") is None:
        assert same_index(by_row, want[0]) and same_index(by_col, want[1])
    else:
        raw = reference_indexes(gold, s, in_cols, "raw")
        plain = cref.read_table(data, kw.get("sep", ","), in_cols, None, kind, kw.get("null_thresh"), kw.get("rownames"))
        assert same_index(plain[0], raw[0]) and same_index(plain[1], raw[1])
        assert same_after_power(by_row, raw[0], want[0], kw["inv_log"]) and same_after_power(by_col, raw[1], want[1], kw["inv_log"])
    genes, cells = [str(x) for x in gold[s + "_genes"]], [str(x) for x in gold[s + "_cells"]]
    assert (genes, cells) == ((cols, rows) if in_cols else (rows, cols))
    meta = json.loads(str(gold["meta"]))[s]
    assert meta["dtype"] == ("[('idx', '<i8'), ('val', '<i8')]" if kind else "[('idx', '<i8'), ('val', '<f8')]")
    assert meta["stats"]["fields"] == 4800 and meta["stats"]["deferred"] == 0 and 0.8 < 1 - meta["stats"]["entries"] / 4800 < 0.9
    if s == "A":
        assert "DUP" in genes and "DUP_2" in genes and "DUP_3" in genes and "XY_2" in genes and cells[0] == "CELL_A0" and 0 in np.diff(by_row[0]) and 0 in np.diff(by_col[0])
    if s == "B":
        assert data.count(b"\t") > 4000 and max(len(f) for f in data.split(b"\n")[1].split(b"\t")) >= 17
    if s == "C":
        assert int(by_row[2].max()) == 2 ** 40 + 7


TABLES = [
    # (body, keyword arguments of parse, the entries (row, col, value) or (line, field, code))
    (b"a,1,0,2\nb,0,0,3\n", dict(n_cols=3), [(0, 0, 1.0), (0, 2, 2.0), (1, 2, 3.0)]),
    (b"a,1,0,2\r\nb,0,0,3\r\n", dict(n_cols=3), [(0, 0, 1.0), (0, 2, 2.0), (1, 2, 3.0)]),
    (b"a,1,0,2\nb,0,0,3", dict(n_cols=3), [(0, 0, 1.0), (0, 2, 2.0), (1, 2, 3.0)]),
    (b"a,1,0,2\nb,0,0,3\r", dict(n_cols=3), [(0, 0, 1.0), (0, 2, 2.0), (1, 2, 3.0)]),
    (b"a,1,0,2\nb,0,0,3\n\n\r\n\n", dict(n_cols=3), [(0, 0, 1.0), (0, 2, 2.0), (1, 2, 3.0)]),
    (b"1;0;2\n0;0;3\n", dict(n_cols=3, has_names=False, sep=b";"), [(0, 0, 1.0), (0, 2, 2.0), (1, 2, 3.0)]),
    (b"x\t nan\t-inf\t-0.0\t1e-400\n", dict(n_cols=4, sep=b"\t"), [(0, 0, float("nan")), (0, 1, float("-inf"))]),
    (b"x,0.5,nan,2,-1\n", dict(n_cols=4, thresh=1.0), [(0, 1, float("nan")), (0, 2, 2.0)]),
    (b"x,5,-7\ny,0,9223372036854775807\n", dict(n_cols=2, kind=1), [(0, 0, 5), (0, 1, -7), (1, 1, 2 ** 63 - 1)]),
    (b"", dict(n_cols=2), []),
    (b"\n\n", dict(n_cols=2), []),
    (b"a,1,2\nb,1\nc,x,1\n", dict(n_cols=2), (2, 3, cref.TOO_FEW)),
    (b"a,1,2\nb,1,2,3\nc,1\n", dict(n_cols=2), (2, 4, cref.TOO_MANY)),
    (b"a,1,2\nb,,2\nc,1\n", dict(n_cols=2), (2, 2, cref.EMPTY)),
    (b"a,1,2\nb,1,2x\nc,1\n", dict(n_cols=2), (2, 3, cref.BAD)),
    (b"a,1,2\nb,1,2.5\nc,1\n", dict(n_cols=2, kind=1), (2, 3, cref.FLOAT)),
    (b"a,1,2\n\nc,1,2\nd,1\n", dict(n_cols=2), (2, 1, cref.EMPTY_LINE)),
    (b"a,1,2\nb,1,\n", dict(n_cols=2), (2, 3, cref.EMPTY)),
    (b"a,1,2\nb,1,2,\n", dict(n_cols=2), (2, 4, cref.TOO_MANY)),
    (b"a,1,2\n" + b"n" * 1025 + b",1,2\n", dict(n_cols=2), (2, 1, cref.NAME_LONG)),
    (b"a,1,2\nb,1,99999999999999999999\n", dict(n_cols=2, kind=1), (2, 3, cref.RANGE)),
]


def test_restatement_on_tables_by_hand():
    for body, kw, want in TABLES:
        for first in (0, 3):
            try:
                p = cref.parse(body, first_line=first, **kw)
            except cref.Refused as e:
                assert (e.line, e.field, e.code) == (want[0] + first, want[1], want[2]), body
                continue
            kind = kw.get("kind", 0)
            val = p["bits"].view(np.int64 if kind else np.float64)
            got = list(zip(p["row"].tolist(), p["col"].tolist(), val.tolist()))
            assert len(got) == len(want) and all(a[:2] == b[:2] and (a[2] == b[2] or (a[2] != a[2] and b[2] != b[2])) for a, b in zip(got, want)), body
    p = cref.parse(b"a,1,0\nb,2,3\n", n_cols=2)
    (row_ptr, col, val), (col_ptr, row, cval) = cref.indexes(p)
    assert row_ptr.tolist() == [0, 1, 3] and col.tolist() == [0, 0, 1] and val.tolist() == [1, 2, 3]
    assert col_ptr.tolist() == [0, 2, 3] and row.tolist() == [0, 1, 1] and cval.tolist() == [1, 2, 3] and p["names"] == ["a", "b"]
    assert p["stats"] == dict(fields=4, entries=3, converted=4, deferred=0)
    long_number = b"0" * 300 + b"7"
    p = cref.parse(b"a," + long_number + b",12345678901234567890\n", n_cols=2)
    assert p["stats"] == dict(fields=2, entries=2, converted=0, deferred=2) and p["bits"].view(np.float64).tolist() == [7.0, 12345678901234567890.0]


def test_names_as_the_reference_reads_them():
    assert cref.header_names(b'"Gene",\'c1\',C1,x\r', ",") == ["GENE", "C1", "C1", "X"] == _csv.header_names(b'"Gene",\'c1\',C1,x\r', ",")
    for given in (False, True):
        for conv in (None, {"C1": "renamed"}):
            names = ["GENE", "C1", "C1", "X"]
            assert cref.column_names(names, given, conv) == _csv.column_names(names, given, conv)
    assert _csv.column_names(["GENE", "C1", "C1", "X"], False) == ["C1_1", "C1_2", "X"] and _csv.column_names(["A", "B"], True, {"A": "b"}) == ["B_1", "B_2"]
    raw = ['"a"', "A", "'b'", "a", "c"]
    assert cref.file_row_names(raw) == ["A", "A_2", "B", "A_3", "C"] == _csv.file_row_names(raw)
    assert cref.file_row_names(raw, {"C": "a"}) == ["A", "A_2", "B", "A_3", "A_4"] == _csv.file_row_names(raw, {"C": "a"})


def test_library_exports_csv_symbols():
    src = open(os.path.join(REPO, "include", "nabo_csv.h")).read()
    assert '#include "nabo_knn.h"' in src
    for other in ("nabo_knn.h", "nabo_ingest.h", "nabo_counts.h"):
        assert "nabo_csv.h" not in open(os.path.join(REPO, "include", other)).read()
    for phrase in ("1_0", "Unicode", "atomicMin", "Clinger", "Eisel-Lemire", "[-27, 55]", "DEFERRED", "2^32 - 1"):
        assert phrase in src, phrase
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert sorted(set(re.findall(r"\b(nabo_[a-z0-9_]+)\s*\(", src))) == sorted(_lib.CSV_SYMBOLS)
    others = (_lib.SYMBOLS + _lib.GRAPH_SYMBOLS + _lib.CLUSTER_SYMBOLS + _lib.DE_SYMBOLS + _lib.PCA_SYMBOLS + _lib.PCA_FIT_SYMBOLS + _lib.QC_SYMBOLS
              + _lib.LAYOUT_SYMBOLS + _lib.UMAP_SYMBOLS + _lib.UMAP_TRANSFORM_SYMBOLS + _lib.COMMUNITY_SYMBOLS + _lib.AGGLOM_SYMBOLS + _lib.POTENTIAL_SYMBOLS
              + _lib.BUNDLE_SYMBOLS + _lib.RENDER_SYMBOLS + _lib.INGEST_SYMBOLS + _lib.COUNTS_SYMBOLS)
    assert not set(_lib.CSV_SYMBOLS) & set(others)
    L = _lib.lib()
    for n in _lib.CSV_SYMBOLS:
        assert hasattr(L, n), n


def test_public_names_geometry_and_signatures():
    import inspect
    for n in ("CsvReader", "CsvMatrix", "read_csv", "csv_to_h5"):
        assert n in nabo_amd.__all__ and callable(getattr(nabo_amd, n))
    g = _csv.geometry()
    host = open(os.path.join(REPO, "nabo_amd", "csrc", "csv_host.h")).read()
    assert "TILE_BYTES = %d, MAX_FIELD = %d, MAX_NAME = %d, HARD_FIELD = %d;" % (g["tile_bytes"], g["max_field"], g["max_name"], cref.HARD_FIELD) in host
    assert (g["max_field"], g["max_name"]) == (cref.MAX_FIELD, cref.MAX_NAME) and g["tile_bytes"] % 64 == 0
    assert "#include <hip" not in host and not re.search(r"\bhip[A-Z]", host)
    assert list(inspect.signature(nabo_amd.csv_to_h5).parameters) == ["csv_fn", "h5_fn", "sep", "genes_in_columns", "inv_log", "value_dtype", "null_thresh", "batch_size",
                                                                      "rownames", "colnames", "colname_converter", "rowname_converter", "skip_lines"]
    assert inspect.signature(nabo_amd.csv_to_h5).parameters["batch_size"].default == 500
    assert inspect.signature(nabo_amd._ingest.write_dataset_file).parameters["idx_dtype"].default is np.uint
    doc = " ".join((_csv.__doc__ + _csv.read_csv.__doc__).split())
    assert "1_0" in doc and "digits outside ASCII" in doc and "departure" in doc.lower()
    m = _csv.CsvMatrix(2, 3, np.array([0, 1, 2]), np.array([2, 0], np.int32), np.array([1.5, 2.5]), np.array([0, 1, 1, 2]), np.array([1, 0], np.int32), np.array([2.5, 1.5]))
    a, b = m.counts(False), m.counts(True)
    assert (a.n_genes, a.n_cells, b.n_genes, b.n_cells) == (2, 3, 3, 2) and a.gene_ptr is m.row_ptr and a.cell_ptr is m.col_ptr and b.cell_ptr is m.row_ptr
    assert a.csr()[2].dtype == np.float32 and a.max_value == 2.5 and a.nnz == 2


def test_arguments_are_checked_before_any_device():
    L, h = _lib.lib(), C.c_void_p()
    for sep in (ord("\n"), ord("\r"), ord("5"), -1, 256):
        assert L.nabo_csv_create(0, sep, 3, 1, 0, 0, 0.0, 0, 0, C.byref(h)) == _lib.E_INVALID and not h.value
    assert L.nabo_csv_create(0, 44, 0, 1, 0, 0, 0.0, 0, 0, C.byref(h)) == _lib.E_INVALID
    assert L.nabo_csv_create(0, 44, 3, 1, 2, 0, 0.0, 0, 0, C.byref(h)) == _lib.E_INVALID
    assert L.nabo_csv_create(0, 44, 3, 1, 0, 1, float("nan"), 0, 0, C.byref(h)) == _lib.E_INVALID
    assert L.nabo_csv_create(0, 44, 3, 1, 0, 0, 0.0, 0, 0, None) == _lib.E_INVALID
    assert L.nabo_csv_feed(None, b"x", 1) == _lib.E_INVALID and L.nabo_csv_finish(None, None, None) == _lib.E_INVALID
    assert L.nabo_csv_geometry(None, None, None) == _lib.E_INVALID and L.nabo_csv_stats(None, None) == _lib.E_INVALID
    L.nabo_csv_free(None)
    with pytest.raises(ValueError):
        nabo_amd.CsvReader(sep=",,")
    with pytest.raises(ValueError):
        nabo_amd.CsvReader(value_dtype=np.float32)


def test_no_device_is_a_loud_failure(gold):
    if nabo_amd.device_count() > 0:
        pytest.skip("a GPU is visible here; the no-device path is covered on the CPU box")
    with pytest.raises(nabo_amd.NaboError) as e:
        nabo_amd.read_csv(io.BytesIO(gold["A_csv"].tobytes()))
    assert "no HIP device" in str(e.value)
    h = C.c_void_p()
    assert _lib.lib().nabo_csv_create(0, 44, 3, 1, 0, 0, 0.0, 0, 0, C.byref(h)) == _lib.E_NODEVICE


# ---- the host half and the shared number routine under the sanitizers ---------------------------------------------------
@pytest.fixture(scope="module")
def host_main(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("csv_host") / "csv_host_main")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(REPO, "tests", "abi_c", "csv_host_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0, r.stdout
    return exe


def run_fields(exe, fields, kind):
    r = subprocess.run([exe, "fields", str(kind)], input=b"".join(f + b"\n" for f in fields), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    out = r.stdout.decode().splitlines()
    assert len(out) == len(fields)
    return out


def said(code, bits):
    return "%d %016x" % (code, bits or 0)


def test_number_routine_equals_the_restatement(host_main, strings):
    fields = [s.encode("latin-1") for s in strings + REFUSED if "\n" not in s] + [b"0" * 300 + b"7", b"1" * 300, b" " * 300 + b"x", b"9" * 5000]
    got = run_fields(host_main, fields, 0)
    for f, g in zip(fields, got):
        if len(f) > cref.HARD_FIELD:
            assert g.startswith("-1 ") and g.endswith("!%d" % cref.FIELD_LONG), f[:20]
            continue
        code, bits = cref.convert(f, False, 0)
        # a field the device would leave to the host for its length, and the host then refuses
        want = said(code, bits) if not (code > 0 and len(f) > cref.MAX_FIELD) else "-1 %016x !%d" % (0, code)
        assert g == want, (f[:40], g, want)
    ints = [b"0", b"-0", b"+17", b"  42 ", b"000123", b"999999999999999999", b"-999999999999999999", b"1000000000000000000", b"9223372036854775807",
            b"-9223372036854775808", b"9223372036854775808", b"-9223372036854775809", b"1.0", b"1e3", b"inf", b"", b"x", b"1_0", b"0" * 300 + b"5"]
    for f, g in zip(ints, run_fields(host_main, ints, 1)):
        code, bits = cref.convert(f, False, 1)
        assert g == (said(code, bits) if code != cref.RANGE else "-1 %016x !%d" % (0, cref.RANGE)), (f, g)


def test_powers_of_five_built_by_the_host(host_main):
    r = subprocess.run([host_main, "table"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = [ln.split() for ln in r.stdout.decode().splitlines()]
    assert [int(q) for q, _, _ in rows] == list(range(-342, 309))
    assert all(cref.POW5[int(q)] == (int(hi, 16) << 64 | int(lo, 16)) for q, hi, lo in rows)


@pytest.mark.parametrize("split", [1, 7, 0])
@pytest.mark.parametrize("chunk", [64, 4096, 0])
def test_host_half_reassembles_the_golden_file(gold, host_main, split, chunk):
    data = gold["B_csv"].tobytes()
    r = subprocess.run([host_main, "feed", str(split), str(chunk), "9"], input=data, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    assert r.stdout == data
    # where the middle of every piece lies, by the carried column: against a count over the whole file
    at = 0
    for ln in r.stderr.decode().splitlines():
        col0, size, line, field = (int(x) for x in ln.split())
        end = at + size
        assert data[end - 1:end] in (b"\t", b"\n")
        mid = at + (end - at) // 2
        start = data.rfind(b"\n", 0, mid) + 1
        assert line == data.count(b"\n", at, mid) and field == data.count(b"\t", start, mid), (at, end)
        assert col0 == data.count(b"\t", data.rfind(b"\n", 0, at) + 1, at)
        at = end
    assert at == len(data)


def test_host_half_on_edges(host_main):
    def feed(data, split, chunk, sep=44):
        r = subprocess.run([host_main, "feed", str(split), str(chunk), str(sep)], input=data, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
        return r.stdout
    for data in (b"", b"\n", b"a,1,2", b"a,1,2\r", b"a,1,2\n\n\n", b"a,,\n,\n"):
        for split in (1, 3, 0):
            assert feed(data, split, 64) == (data if data.endswith(b"\n") or not data else data + b"\n")
    # a field that outgrows the buffer: 4096 bytes pass, one more does not
    ok, over = b"a," + b"1" * 4096 + b",2\n", b"a," + b"1" * 4097 + b",2\n"
    assert feed(ok, 50, 64) == ok and feed(over, 50, 64) == b"a,too long\n"
