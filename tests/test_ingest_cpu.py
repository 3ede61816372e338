"""The Matrix Market reader (include/nabo_ingest.h, nabo_amd/_ingest.py) without a GPU: the C header and its symbols,
the plain restatement (tests/_ingest_ref.py) against what the reference wrote (tests/golden/ingest.npz,
tools/gen_golden_ingest.py) and against cases written by hand, the readers of gene names and barcodes, the argument
checks of the transpose, the no-device failure, and the host half of the reader (nabo_amd/csrc/mtx_host.h: header parser,
line buffer, the host's statement of a line) built with a small main under the address and undefined-behaviour
sanitizers as a program of its own."""
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

import nabo_amd
from nabo_amd import _ingest, _lib

import _ingest_ref as iref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_LINE = 1024
HEAD = b"%%MatrixMarket matrix coordinate integer general\n"


def build_ingest_check(tmp_path):
    exe = os.path.join(str(tmp_path), "ingest_check")
    cmd = ["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(REPO, "include"),
           os.path.join(REPO, "tests", "abi_c", "ingest_check.c"), "-L" + os.path.join(REPO, "nabo_amd"), "-lnabo_knn",
           "-Wl,-rpath," + os.path.join(REPO, "nabo_amd"), "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0, r.stdout
    return exe


def files_of(d, s):
    """{file name: bytes} of a golden directory"""
    pre = s + "_file_"
    return {k[len(pre):]: d[k].tobytes() for k in d.files if k.startswith(pre)}


def write_dir(d, s, where):
    os.makedirs(str(where), exist_ok=True)
    for name, data in files_of(d, s).items():
        with open(os.path.join(str(where), name), "wb") as f:
            f.write(data)
    return str(where)


def mtx_bytes(d, s):
    f = files_of(d, s)
    return f["matrix.mtx"] if "matrix.mtx" in f else gzip.decompress(f["matrix.mtx.gz"])


def reference_indexes(d, s):
    """((cell_ptr, gene, val), (gene_ptr, cell, gene_val)) from the records the reference wrote; a cell without a
    dataset has no entries"""
    has = d[s + "_cell_has_dataset"]
    n = np.zeros(has.shape[0], dtype=np.int64)
    n[has] = d[s + "_cell_len"]
    cell_ptr, gene_ptr = np.zeros(has.shape[0] + 1, np.int64), np.zeros(d[s + "_gene_len"].shape[0] + 1, np.int64)
    np.cumsum(n, out=cell_ptr[1:])
    np.cumsum(d[s + "_gene_len"], out=gene_ptr[1:])
    return ((cell_ptr, d[s + "_cell_idx"].astype(np.int32), d[s + "_cell_val"].astype(np.uint32)),
            (gene_ptr, d[s + "_gene_idx"].astype(np.int32), d[s + "_gene_val"].astype(np.uint32)))


def same_index(a, b):
    return all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def gold(golden):
    return golden("ingest")


def test_header_is_plain_c_and_links(tmp_path):
    _lib.lib()
    exe = build_ingest_check(tmp_path)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0 and "%d entry points" % len(_lib.INGEST_SYMBOLS) in r.stdout, r.stdout


def test_library_exports_ingest_symbols():
    src = open(os.path.join(REPO, "include", "nabo_ingest.h")).read()
    assert '#include "nabo_knn.h"' in src
    assert "nabo_ingest.h" not in open(os.path.join(REPO, "include", "nabo_knn.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert sorted(set(re.findall(r"\b(nabo_[a-z0-9_]+)\s*\(", src))) == sorted(_lib.INGEST_SYMBOLS)
    others = (_lib.SYMBOLS + _lib.GRAPH_SYMBOLS + _lib.CLUSTER_SYMBOLS + _lib.DE_SYMBOLS + _lib.PCA_SYMBOLS + _lib.PCA_FIT_SYMBOLS
              + _lib.QC_SYMBOLS + _lib.LAYOUT_SYMBOLS + _lib.UMAP_SYMBOLS + _lib.UMAP_TRANSFORM_SYMBOLS + _lib.COMMUNITY_SYMBOLS
              + _lib.AGGLOM_SYMBOLS + _lib.POTENTIAL_SYMBOLS + _lib.BUNDLE_SYMBOLS + _lib.RENDER_SYMBOLS)
    assert not set(_lib.INGEST_SYMBOLS) & set(others)
    L = _lib.lib()
    for n in _lib.INGEST_SYMBOLS:
        assert hasattr(L, n), n


def test_public_names_and_geometry():
    for n in ("MtxReader", "CountMatrix", "read_mtx", "mtx_to_h5", "csr_to_csc", "fix_dup_names"):
        assert n in nabo_amd.__all__ and callable(getattr(nabo_amd, n))
    g = _ingest.geometry()
    host = open(os.path.join(REPO, "nabo_amd", "csrc", "mtx_host.h")).read()
    assert "TILE_BYTES = %d, MAX_LINE = %d;" % (g["tile_bytes"], g["max_line"]) in host
    assert g["max_line"] == MAX_LINE and g["tile_bytes"] % 64 == 0 and g["tile_bytes"] > g["max_line"]
    doc = " ".join((_ingest.CountMatrix.__doc__ + _ingest.read_mtx.__doc__).split())
    assert "NOT exact in float32" in doc and "bound by the host's inflate" in doc


@pytest.mark.parametrize("s", ["A", "B"])
def test_restatement_reproduces_the_reference(gold, s):
    parsed = iref.parse(mtx_bytes(gold, s), MAX_LINE)
    csr, csc = iref.csr_csc(parsed)
    want_csr, want_csc = reference_indexes(gold, s)
    assert parsed[0] == 200 and parsed[1] == 300 and len(parsed[2]) > 5000
    assert same_index(csr, want_csr) and same_index(csc, want_csc)
    assert int(csr[2].max()) > 2 ** 31
    has, n_ent = gold[s + "_cell_has_dataset"], np.diff(csr[0])
    assert has[n_ent > 0].all() and (n_ent == 0).sum() == 3 and has[0] and (~has).sum() == 2       # the accident of cell 1
    # the transpose of the one is the other
    t = iref.transpose(csr[0], csr[1], csr[2].astype(np.float32), parsed[0])
    assert np.array_equal(t[0], csc[0]) and np.array_equal(t[1], csc[1]) and np.array_equal(t[2], csc[2].astype(np.float32))


LINES = [
    (b"1 1 1", (1, 1, 1)), (b"  3\t 2   7 \t", (3, 2, 7)), (b"003 0002 0", (3, 2, 0)), (b"3 2 7\r", (3, 2, 7)), (b"", None), (b" \t ", None), (b"\r", None),
    (b"% 1 2 x", None), (b"  %", None), (b"5 9 4294967295", (5, 9, 4294967295)), (b"5 9 4294967296", iref.VALUE), (b"5 9 0000000000000000000000001", (5, 9, 1)),
    (b"5 9 1000000000000000000000000", iref.VALUE), (b"1000000000000000000000000 9 1", iref.GENE), (b"0 1 1", iref.GENE), (b"6 1 1", iref.GENE),
    (b"1 10 1", iref.CELL), (b"1 0 1", iref.CELL), (b"-1 1 1", iref.SYNTAX), (b"1 1 3.0", iref.REAL), (b"1 1 1e3", iref.REAL), (b"1 1 .5", iref.REAL),
    (b"1 1 e3", iref.SYNTAX), (b"1 1", iref.FIELDS), (b"1 1 1 1", iref.FIELDS), (b"1 1 1 x", iref.SYNTAX), (b"1 1 +1", iref.SYNTAX), (b"1 1\r 1", iref.SYNTAX),
    (b"1 % 1", iref.SYNTAX), (b"9 9 9 " + b" " * (MAX_LINE - 6), iref.GENE), (b"1 1 1" + b" " * (MAX_LINE - 5), (1, 1, 1)), (b"1 1 1" + b" " * (MAX_LINE - 4), iref.LONG),
    (b"%" + b"x" * MAX_LINE, iref.LONG), (b"18446744073709551617 1 1", iref.GENE), (b"1 1 9999999999999999999", iref.VALUE),
]


def test_restatement_on_lines_by_hand():
    for line, want in LINES:
        assert iref.parse_line(line, 5, 9, MAX_LINE) == want, line


def test_restatement_on_files_by_hand():
    size = b"5 9 2\n"
    ok = iref.parse(HEAD + b"%c\n" + size + b"1 1 1\n\n% x\n2 9 3", MAX_LINE)
    assert ok[2].tolist() == [0, 1] and ok[3].tolist() == [0, 8] and ok[4].tolist() == [1, 3]
    for data, status, line in ((b"%MatrixMarket matrix coordinate integer general\n" + size, -1, 1), (HEAD.replace(b"general", b"symmetric") + size, -1, 1),
                               (HEAD.replace(b"integer", b"complex") + size, -1, 1), (HEAD + b"%\n5 9\n", -1, 3), (HEAD + b"5 9 -2\n", -1, 2),
                               (HEAD + b"2147483648 9 2\n", -5, 2), (HEAD + b"5 2147483648 2\n", -5, 2), (HEAD, -1, 2), (b"", -1, 1),
                               (HEAD + size + b"1 1 1\n1 1 x\n0 0 0\n", -1, 4), (HEAD + size + b"1 1 1\n2 1 1\n3 1 1\n", -1, 5),
                               (HEAD + size + b"1 1 1\n\n", -1, 4), (HEAD + size + b"1 1 1\n1 1 2\n", -1, None)):
        with pytest.raises(iref.Refused) as e:
            iref.parse(data, MAX_LINE)
        assert (e.value.status, e.value.line) == (status, line), data
    up = iref.parse(HEAD.upper().replace(b"%%MATRIXMARKET", b"%%MatrixMarket").replace(b"INTEGER", b"Real") + b"5 9 0", MAX_LINE)
    assert up[:2] == (5, 9) and len(up[2]) == 0


def test_names_as_the_reference_reads_them(gold, tmp_path):
    assert iref.fix_dup_names(["a", "B", "A", "b", "c", "a"]) == ["A_1", "B_1", "A_2", "B_2", "C", "A_3"] == nabo_amd.fix_dup_names(["a", "B", "A", "b", "c", "a"])
    for s in ("A", "B"):
        where = write_dir(gold, s, tmp_path / s)
        genes, fn = _ingest.read_gene_names(where)
        assert genes == [str(x) for x in gold[s + "_genes"]] and fn == ("genes.tsv" if s == "A" else "features.tsv.gz")
        assert _ingest.read_barcodes(where) == [str(x) for x in gold[s + "_cells"]]
        assert len(set(genes)) == len(genes) and "ABC1_3" in genes and "XY_2" in genes and genes[0] == "GENE0"
    with pytest.raises(FileNotFoundError):
        _ingest.read_gene_names(str(tmp_path))
    with pytest.raises(FileNotFoundError):
        _ingest.read_barcodes(str(tmp_path))


GOOD = dict(ptr=[0, 2, 3], idx=[0, 2, 1], val=[1.0, 2.0, 3.0], n_cols=3)


@pytest.mark.parametrize("change", [
    {"ptr": [0, 4, 3]},                                       # not monotone
    {"ptr": [1, 2, 3]},                                       # ptr[0] != 0
    {"idx": [0, 3, 1]},                                       # an index out of range
    {"idx": [0, -1, 1]},
    {"idx": [2, 0, 1]},                                       # a row that is not increasing
    {"idx": [1, 1, 0]},                                       # an index twice in a row
    {"val": [1.0, np.nan, 3.0]},
    {"val": [1.0, -2.0, 3.0]},
    {"val": [1.0, 2.0]},
    {"n_cols": -1},
])
def test_transpose_refuses_bad_arguments_before_any_device(change):
    with pytest.raises(ValueError) as e:
        nabo_amd.csr_to_csc(**dict(GOOD, **change))
    assert str(e.value).startswith("ERROR: ")


def test_no_device_is_a_loud_failure(gold):
    if nabo_amd.device_count() > 0:
        pytest.skip("a GPU is visible here; the no-device path is covered on the CPU box")
    import io
    with pytest.raises(nabo_amd.NaboError) as e:
        nabo_amd.read_mtx(io.BytesIO(mtx_bytes(gold, "A")))
    assert "no HIP device" in str(e.value)
    with pytest.raises(nabo_amd.NaboError) as e:
        nabo_amd.csr_to_csc(**GOOD)
    assert "no HIP device" in str(e.value)


# ---- the host half under the sanitizers -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_main(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mtx_host") / "mtx_host_main")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(REPO, "tests", "abi_c", "mtx_host_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0, r.stdout
    return exe


def run_host(exe, data, split, chunk):
    r = subprocess.run([exe, str(split), str(chunk)], input=data, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    first, _, rest = r.stdout.partition(b"\n")
    return first.decode(), rest, [int(x) for x in r.stderr.split()]


@pytest.mark.parametrize("split", [1, 7, 0])
@pytest.mark.parametrize("chunk", [64, 0])
def test_host_half_reassembles_the_golden_file(gold, host_main, split, chunk):
    data = mtx_bytes(gold, "A")
    n_genes, n_cells, nnz, n_head, pos = iref.parse_header(data)
    first, body, verdicts = run_host(host_main, data, split, chunk)
    assert first == "header %d %d %d %d 0" % (n_genes, n_cells, nnz, n_head) and n_head == 4
    assert body == data[pos:] and verdicts == [0] * nnz


def test_host_half_on_a_messy_file(host_main):
    body = b"\n".join(line for line, _ in LINES if len(line) <= MAX_LINE)
    data = HEAD.replace(b"integer", b"REAL") + b"%a\r\n% b\n  5\t9 0007  \r\n" + body + b"\r"
    want = [iref.parse_line(line, 5, 9, MAX_LINE) for line in (body + b"\r").split(b"\n")]
    want = [0 if isinstance(w, tuple) else -1 if w is None else w for w in want]
    for split in (1, 3, 0):
        first, got, verdicts = run_host(host_main, data, split, 64)
        assert first == "header 5 9 7 4 1" and got == body + b"\r\n" and verdicts == want
    # the codes are the restatement's
    assert {iref.SYNTAX, iref.REAL, iref.FIELDS, iref.GENE, iref.CELL, iref.VALUE, 0, -1} <= set(want)
    # a line that outgrows the buffer, and refusals of the header
    first, got, _ = run_host(host_main, HEAD + b"5 9 1\n1 1 1\n" + b"1" * (MAX_LINE + 1), 5, 64)
    assert first == "header 5 9 1 2 0" and got == b"1 1 1\ntoo long\n"
    for data, status, line in ((b"%%MatrixMarket matrix array integer general\n1 1 1\n", -1, 1), (HEAD + b"% c\n5 9\n", -1, 3), (HEAD + b"5 2147483648 1\n", -5, 2),
                               (HEAD + b"5 9 4294967295\n", -5, 2), (HEAD + b"%x", -1, 3), (b"", -1, 1)):
        for split in (1, 0):
            first = run_host(host_main, data, split, 64)[0]
            assert first.startswith("refused %d line %d:" % (status, line)), (data, first)
    assert run_host(host_main, HEAD + b"5 9 0", 1, 64)[0] == "header 5 9 0 2 0"
