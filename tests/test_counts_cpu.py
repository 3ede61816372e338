"""The Matrix Market writer and the remap of count matrices (include/nabo_counts.h, nabo_amd/_counts.py) without a GPU:
the C header and its symbols, the public names, the plain restatement (tests/_counts_ref.py) against what the reference
wrote (tests/golden/counts.npz, tools/gen_golden_counts.py) and against cases written out by hand, the argument checks,
the no-device failure, and the host half (nabo_amd/csrc/counts_host.h: the text in front of the body, digits and lines,
the index check, the remap's plan, the serving of bytes in any cap) built with a small main under the address and
undefined-behaviour sanitizers as a program of its own."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import nabo_amd
from nabo_amd import _counts, _lib

import _counts_ref as cref
import _ingest_ref as iref
from test_ingest_cpu import mtx_bytes

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMMENT = b'%metadata_json: {"format_version": 2, "software_version": "3.0.2"}\n'
E_INVALID, E_NODEVICE, E_NOMEM, E_UNSUPPORTED = -1, -2, -4, -5


def build_counts_check(tmp_path):
    exe = os.path.join(str(tmp_path), "counts_check")
    cmd = ["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(REPO, "include"),
           os.path.join(REPO, "tests", "abi_c", "counts_check.c"), "-L" + os.path.join(REPO, "nabo_amd"), "-lnabo_knn",
           "-Wl,-rpath," + os.path.join(REPO, "nabo_amd"), "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0, r.stdout
    return exe


def golden_matrix(ingest, s):
    """(n_genes, csr, csc, genes, cells) of a golden directory of ingest.npz, restated"""
    parsed = iref.parse(mtx_bytes(ingest, s), 1024)
    csr, csc = iref.csr_csc(parsed)
    return parsed[0], csr, csc, [str(x) for x in ingest[s + "_genes"]], [str(x) for x in ingest[s + "_cells"]]


def records(d, pre):
    return d[pre + "_len"], d[pre + "_idx"], d[pre + "_val"]


def same_records(got, index):
    """(lengths, idx, val) of a golden against a (ptr, idx, val)"""
    return all(np.array_equal(np.asarray(a).astype(np.int64), np.asarray(b).astype(np.int64)) for a, b in zip(got, (np.diff(index[0]), index[1], index[2])))


@pytest.fixture(scope="module")
def gold(golden):
    return golden("counts")


@pytest.fixture(scope="module")
def ingest(golden):
    return golden("ingest")


def test_header_is_plain_c_and_links(tmp_path):
    _lib.lib()
    exe = build_counts_check(tmp_path)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0 and "%d entry points" % len(_lib.COUNTS_SYMBOLS) in r.stdout, r.stdout


def test_library_exports_counts_symbols():
    src = open(os.path.join(REPO, "include", "nabo_counts.h")).read()
    assert '#include "nabo_knn.h"' in src
    for other in ("nabo_knn.h", "nabo_ingest.h"):
        assert "nabo_counts.h" not in open(os.path.join(REPO, "include", other)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert sorted(set(re.findall(r"\b(nabo_[a-z0-9_]+)\s*\(", src))) == sorted(_lib.COUNTS_SYMBOLS)
    others = (_lib.SYMBOLS + _lib.GRAPH_SYMBOLS + _lib.CLUSTER_SYMBOLS + _lib.DE_SYMBOLS + _lib.PCA_SYMBOLS + _lib.PCA_FIT_SYMBOLS
              + _lib.QC_SYMBOLS + _lib.LAYOUT_SYMBOLS + _lib.UMAP_SYMBOLS + _lib.UMAP_TRANSFORM_SYMBOLS + _lib.COMMUNITY_SYMBOLS
              + _lib.AGGLOM_SYMBOLS + _lib.POTENTIAL_SYMBOLS + _lib.BUNDLE_SYMBOLS + _lib.RENDER_SYMBOLS + _lib.INGEST_SYMBOLS
              + _lib.INSPECT_SYMBOLS)
    assert not set(_lib.COUNTS_SYMBOLS) & set(others)
    L = _lib.lib()
    for n in _lib.COUNTS_SYMBOLS:
        assert hasattr(L, n), n
    for n in ("nabo_mtxw_create", "nabo_mtxw_read", "nabo_mtxw_last_device_ms", "nabo_mtxw_free", "nabo_counts_remap"):
        assert n in _lib.COUNTS_SYMBOLS


def test_public_names_and_geometry():
    for n in ("MtxWriter", "write_mtx", "remap_counts", "read_h5_counts", "subset_cells", "merge_counts", "extract_cells_from_h5", "merge_h5", "h5_to_mtx"):
        assert n in nabo_amd.__all__ and callable(getattr(nabo_amd, n))
    g = _counts.writer_geometry()
    host = open(os.path.join(REPO, "nabo_amd", "csrc", "counts_host.h")).read()
    assert "TILE_BYTES = %d, LONG_CELL = %d, MAX_LINE = %d;" % (g["tile_bytes"], g["long_cell"], g["max_line"]) in host
    assert g["max_line"] == len("4294967295 2147483647 4294967295\n") and g["tile_bytes"] % 16 == 0 and g["min_chunk"] % 16 == 0
    assert g["min_chunk"] < g["tile_bytes"]                     # so that chunk boundaries fall inside tiles in the tests
    doc = " ".join((_counts.merge_h5.__doc__ + _counts.h5_to_mtx.__doc__ + _counts.extract_cells_from_h5.__doc__).split())
    for said in ("sorted union", "seeded permutation", "ascending by index", "read-only", "are refused", "order of the FILE"):
        assert said in doc, said
    import inspect
    assert list(inspect.signature(nabo_amd.extract_cells_from_h5).parameters) == ["in_fn", "out_fn", "coi"]
    assert list(inspect.signature(nabo_amd.h5_to_mtx).parameters) == ["fn", "outdir"]
    assert list(inspect.signature(nabo_amd.merge_h5).parameters)[:3] == ["h5_fns", "merged_fn", "cell_suffixes"]


# ---- the restatement against the reference ------------------------------------------------------------------------
def test_the_reference_ran(gold):
    meta = json.loads(str(gold["meta"]))
    assert meta["h5_to_mtx_A"] is None and meta["h5_to_mtx_B"] is None and meta["extract"] is None and meta["merge"] is None
    assert meta["merge_gene_records_unsorted"] is True          # why the merged gene records are compared after sorting


@pytest.mark.parametrize("s", ["A", "B"])
def test_restatement_reproduces_the_written_files(gold, ingest, s):
    n_genes, csr, _, genes, cells = golden_matrix(ingest, s)
    text = gold[s + "_mtx_file_matrix.mtx"].tobytes()
    assert cref.mtx_text(n_genes, csr[0], csr[1], csr[2], COMMENT, blank=True) == text
    assert text.count(b"\n\n") >= 1 and (np.diff(csr[0]) == 0).sum() == 3
    assert text != cref.mtx_text(n_genes, csr[0], csr[1], csr[2], COMMENT, blank=False)
    # and the reader's restatement reads it back
    back = iref.csr_csc(iref.parse(text, 1024))
    assert all(np.array_equal(a, b) for a, b in zip(back[0], csr))
    assert gold[s + "_mtx_file_genes.tsv"].tobytes() == "".join(g + "\t" + g + "\n" for g in genes).encode()
    assert gold[s + "_mtx_file_barcodes.tsv"].tobytes() == "".join(c + "\n" for c in cells).encode()


def test_restatement_reproduces_the_extracted_file(gold, ingest):
    n_genes, csr, _, genes, cells = golden_matrix(ingest, "A")
    coi = set(str(x) for x in gold["extract_coi"])
    rows = [n for n, c in enumerate(cells) if c in coi]
    assert len(rows) == 100 and len(coi) == 102
    assert [str(c) for c in gold["extract_coi"] if str(c) in cells] != [cells[r] for r in rows]          # coi is not in file order; the output is
    assert [str(x) for x in gold["extract_cells"]] == [cells[r] for r in rows] and [str(x) for x in gold["extract_genes"]] == genes
    want = cref.subset(csr[0], csr[1], csr[2], n_genes, rows)
    assert same_records(records(gold, "extract_cell"), want[0]) and same_records(records(gold, "extract_gene"), want[1])


def test_restatement_reproduces_the_merged_file(gold, ingest):
    a, b = golden_matrix(ingest, "A"), golden_matrix(ingest, "B")
    cells = [str(x) for x in gold["merge_cells"]]
    want = cref.merge([a[1], b[1]], [a[3], b[3]], [a[4], b[4]], ["s1", "s2"], cells)
    assert [str(x) for x in gold["merge_genes"]] == want[2] == sorted(a[3]) and len(cells) == 600
    assert cells != [c + "-s1" for c in a[4]] + [c + "-s2" for c in b[4]]          # the reference shuffled them
    assert same_records(cref.sorted_records(*records(gold, "merge_cell")), want[0])
    assert same_records(cref.sorted_records(*records(gold, "merge_gene")), want[1])
    assert not same_records(records(gold, "merge_gene"), want[1])


def test_restatement_by_hand():
    ptr, gene, val = [0, 2, 2, 3, 3], [0, 4, 2], [7, 0, 4294967295]
    assert cref.mtx_text(5, ptr, gene, val) == cref.BANNER + b"5 4 3\n1 1 7\n5 1 0\n3 3 4294967295\n"
    assert cref.mtx_text(5, ptr, gene, val, b"%a\n%b\n", blank=True) == cref.BANNER + b"%a\n%b\n5 4 3\n1 1 7\n5 1 0\n\n3 3 4294967295\n\n"
    assert cref.mtx_text(3, [0], [], []) == cref.BANNER + b"3 0 0\n"
    # rows 2, 0, 0 with columns reversed and column 2 dropped
    csr, csc = cref.remap(ptr, gene, np.array(val, np.uint32), [2, 0, 0], [4, 3, -1, 1, 0], 5)
    assert csr[0].tolist() == [0, 0, 2, 4] and csr[1].tolist() == [0, 4, 0, 4] and csr[2].tolist() == [0, 7, 0, 7]
    assert csc[0].tolist() == [0, 2, 2, 2, 2, 4] and csc[1].tolist() == [1, 2, 1, 2] and csc[2].tolist() == [0, 0, 7, 7]
    with pytest.raises(cref.Duplicate) as e:
        cref.remap(ptr, gene, np.array(val, np.uint32), [2, 0, 0], [1, 0, 0, 0, 1], 2)
    assert (e.value.row, e.value.col) == (1, 1)
    f = np.array([1.5, -0.0, np.nan], np.float32)
    back = cref.remap(ptr, gene, f, [0, 2], [0, 1, 2, 3, 4], 5)[0][2]
    assert back.dtype == np.float32 and back.tobytes() == f.tobytes()
    m = cref.merge([([0, 1, 2], [0, 1], [5, 6]), ([0, 2], [0, 1], [8, 9])], [["B", "A"], ["C", "A"]], [["x", "y"], ["x"]], ["1", "2"], ["x-2", "y-1", "x-1"])
    assert m[2] == ["A", "B", "C"] and m[0][0].tolist() == [0, 2, 3, 4] and m[0][1].tolist() == [0, 2, 0, 1] and m[0][2].tolist() == [9, 8, 6, 5]
    assert m[1][0].tolist() == [0, 2, 3, 4] and m[1][1].tolist() == [0, 1, 2, 0]


# ---- arguments ------------------------------------------------------------------------------------------------------
GOOD = dict(ptr=[0, 2, 3], idx=[0, 2, 1], val=np.array([1, 2, 3], np.uint32), n_cols=3, row_src=[1, 0], col_map=[2, -1, 0], n_out_cols=3)


@pytest.mark.parametrize("change", [
    {"ptr": [0, 4, 3]},                                       # not monotone
    {"ptr": [1, 2, 3]},                                       # ptr[0] != 0
    {"ptr": [0, 2, 4]},                                       # more entries announced than given
    {"idx": [0, 3, 1]},                                       # an index out of range
    {"idx": [0, -1, 1]},
    {"idx": [2, 0, 1]},                                       # a row that is not increasing
    {"idx": [1, 1, 0]},                                       # an index twice in a row
    {"val": np.array([1, 2], np.uint32)},
    {"val": np.array([1, 2, 3], np.int64)},                   # neither uint32 nor float32
    {"n_cols": -1},
    {"row_src": [0, 2]},                                      # no such row
    {"row_src": [-1]},
    {"col_map": [2, -2, 0]},
    {"col_map": [3, -1, 0]},                                  # no such output column
    {"col_map": [0, 1]},                                      # one entry per input column
    {"n_out_cols": -1},
])
def test_remap_refuses_bad_arguments_before_any_device(change):
    with pytest.raises(ValueError) as e:
        nabo_amd.remap_counts(**dict(GOOD, **change))
    assert str(e.value).startswith("ERROR: ")


@pytest.mark.parametrize("change", [
    {"m": ([0, 4, 3], [0, 2, 1], [1, 2, 3])},
    {"m": ([1, 2, 3], [0, 2, 1], [1, 2, 3])},
    {"m": ([0, 2, 3], [0, 3, 1], [1, 2, 3])},
    {"m": ([0, 2, 3], [2, 0, 1], [1, 2, 3])},
    {"m": ([0, 2, 3], [1, 1, 0], [1, 2, 3])},
    {"m": ([0, 2, 3], [0, 2, 1], [1, -2, 3])},                 # a negative value
    {"m": ([0, 2, 3], [0, 2, 1], [1, 2 ** 32, 3])},            # a value that does not fit
    {"m": ([0, 2, 3], [0, 2, 1], [1.0, 2.5, 3.0])},            # not an integer
    {"m": ([0, 2, 3], [0, 2, 1], [1, 2])},
    {"n_genes": None},
    {"n_genes": 2 ** 31},
    {"comments": "no percent\n"},
    {"comments": "%no newline"},
    {"comments": "%one\nsecond has none\n"},
])
def test_writer_refuses_bad_arguments_before_any_device(change):
    good = dict(m=([0, 2, 3], [0, 2, 1], [1, 2, 3]), n_genes=3, comments="%fine\n% too\n")
    with pytest.raises(ValueError) as e:
        nabo_amd.MtxWriter(**dict(good, **change))
    assert str(e.value).startswith("ERROR: ")


def test_statuses_of_the_c_abi_without_a_device():
    import ctypes as C
    L = _lib.lib()
    ptr, idx, val = np.array([0, 2, 3], np.int64), np.array([0, 2, 1], np.int32), np.array([1, 2, 3], np.uint32)
    h, total = C.c_void_p(), C.c_int64()

    def create(n_genes=3, n_cells=2, ptr=ptr, comments=None):
        return L.nabo_mtxw_create(0, n_genes, n_cells, ptr.ctypes.data, idx.ctypes.data, val.ctypes.data, comments, 0, 0, 0, C.byref(h), C.byref(total))
    assert create(n_genes=2 ** 31) == E_UNSUPPORTED and create(n_genes=-1) == E_INVALID and create(n_cells=-1) == E_INVALID
    assert create(ptr=np.array([0, 2, 2 ** 32 - 1], np.int64)) == E_UNSUPPORTED          # nnz is judged before any entry is read
    assert create(comments=b"x\n") == E_INVALID and h.value is None
    assert L.nabo_mtxw_create(0, 3, 2, ptr.ctypes.data, idx.ctypes.data, val.ctypes.data, None, 0, 0, 0, None, None) == E_INVALID
    buf, n = np.zeros(4, np.uint8), C.c_int64()
    assert L.nabo_mtxw_read(None, buf.ctypes.data, 4, C.byref(n)) == E_INVALID
    src, cmap, nnz = np.array([0], np.int64), np.array([0, 1, 2], np.int32), C.c_int64()
    out = [np.zeros(2, np.int64), np.zeros(2, np.int32), np.zeros(2, np.uint32)]

    def remap(n_rows=2, n_cols=3, n_out_cols=3, out_ptr=out[0].ctypes.data):
        return L.nabo_counts_remap(0, n_rows, n_cols, ptr.ctypes.data, idx.ctypes.data, val.ctypes.data, 1, src.ctypes.data, n_out_cols, cmap.ctypes.data,
                                   C.byref(nnz), out_ptr, out[1].ctypes.data, out[2].ctypes.data, None, None, None)
    assert remap(n_rows=2 ** 31 - 1) == E_UNSUPPORTED and remap(n_out_cols=2 ** 31 - 1) == E_UNSUPPORTED and remap(n_out_cols=2) == E_INVALID
    assert remap(out_ptr=None) == E_INVALID
    # csc_ptr without csc_idx
    assert L.nabo_counts_remap(0, 2, 3, ptr.ctypes.data, idx.ctypes.data, val.ctypes.data, 1, src.ctypes.data, 3, cmap.ctypes.data, C.byref(nnz),
                               out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data, out[0].ctypes.data, None, None) == E_INVALID


def test_no_device_is_a_loud_failure(tmp_path):
    if nabo_amd.device_count() > 0:
        pytest.skip("a GPU is visible here; the no-device path is covered on the CPU box")
    import io
    with pytest.raises(nabo_amd.NaboError) as e:
        nabo_amd.write_mtx(([0, 2, 3], [0, 2, 1], [1, 2, 3]), io.BytesIO(), n_genes=3)
    assert "no HIP device" in str(e.value)
    with pytest.raises(nabo_amd.NaboError) as e:
        nabo_amd.remap_counts(**GOOD)
    assert "no HIP device" in str(e.value)


# ---- the host half under the sanitizers -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_main(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("counts_host") / "counts_host_main")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(REPO, "tests", "abi_c", "counts_host_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0, r.stdout
    return exe


def run_host(exe, n_genes, csr, row_src, col_map, n_out_cols, blank=0, cap=4096, chunk=0, comments=""):
    blob = b"".join([np.array([n_genes, len(csr[0]) - 1, len(row_src), n_out_cols, len(col_map)], np.int64).tobytes(), np.asarray(csr[0], np.int64).tobytes(),
                     np.asarray(csr[1], np.int32).tobytes(), np.asarray(csr[2], np.uint32).tobytes(), np.asarray(row_src, np.int64).tobytes(),
                     np.asarray(col_map, np.int32).tobytes()])
    r = subprocess.run([exe, str(blank), str(cap), str(chunk), comments], input=blob, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    said = {ln.split()[0]: [int(x) for x in ln.split()[1:]] for ln in r.stderr.decode().splitlines()}
    return r.stdout, said


@pytest.mark.parametrize("cap", [1, 7, 100000])
@pytest.mark.parametrize("chunk", [64, 0])
def test_host_half_serves_the_golden_text(gold, ingest, host_main, cap, chunk):
    n_genes, csr, _, _, _ = golden_matrix(ingest, "A")
    text, said = run_host(host_main, n_genes, csr, np.arange(300), np.arange(n_genes), n_genes, blank=1, cap=cap, chunk=chunk, comments=COMMENT.decode())
    assert text == gold["A_mtx_file_matrix.mtx"].tobytes()
    assert said["comments"] == [1] and said["idx"] == [0, 0, 0] and said["digits"] == [1] and said["chunk"] == [64 if chunk else 64 << 20]
    assert said["long"] == [0, int(np.diff(csr[0]).max())] and said["plan"] == [0, 0, len(csr[1]), 1]


def test_host_half_on_edges(host_main):
    # values and genes at every digit boundary, in one cell; empty cells around it
    edge = sorted({0, 2 ** 32 - 1} | {10 ** k + d for k in range(1, 10) for d in (-1, 0)})
    genes = [g - 1 for g in edge if 1 <= g <= 2 ** 31 - 1]
    vals = (edge * 2)[:len(genes)]
    csr = ([0, 0, 0, len(genes), len(genes)], genes, vals)
    for blank in (0, 1):
        text, said = run_host(host_main, 2 ** 31 - 1, csr, [2, 2, 0], np.zeros(0, np.int32), 1, blank=blank, cap=3, chunk=1)
        assert text == cref.mtx_text(2 ** 31 - 1, *csr, blank=bool(blank)) and said["chunk"] == [64] and said["idx"] == [0, 0, 0]
    ptr, idx, val = [0, 3, 3, 5], [0, 1, 3, 1, 2], [1, 2, 3, 4, 5]
    plans = [(([2, 0, 0], [3, 2, 1, 0], 4), [0, 0, 8, 0]), (([2, 0, 0], [0, -1, 1, 1], 2), [0, 0, 8, 1]), (([1, 1], [0, 1, 2, 3], 4), [0, 0, 0, 1]),
             (([0, 3], [0, 1, 2, 3], 4), [1, 1, 0, 0]), (([0], [0, 4, 2, 3], 4), [2, 1, 0, 0]), (([0], [0, -2, 2, 3], 4), [2, 1, 0, 0]), (([], [-1] * 4, 0), [0, 0, 0, 1])]
    for (row_src, col_map, n_out_cols), want in plans:
        _, said = run_host(host_main, 4, (ptr, idx, val), row_src, col_map, n_out_cols)
        assert said["plan"] == want, (row_src, col_map)
    # what the index check says, and where; comments that are no lines; a long cell
    for bad, want in (([0, 1, 4, 1, 2], [2, 0, 2]), ([0, 1, 3, 2, 2], [3, 2, 4]), ([0, 1, -3, 1, 2], [2, 0, 2]), ([1, 0, 3, 1, 2], [3, 0, 1])):
        assert run_host(host_main, 4, (ptr, bad, val), [0], [0] * 4, 1)[1]["idx"] == want
    for comments, ok in (("%a\n", 1), ("%a\n%\n", 1), ("a\n", 0), ("%a", 0), ("%a\n\n", 0)):
        assert run_host(host_main, 4, (ptr, idx, val), [0], [0] * 4, 1, comments=comments)[1]["comments"] == [ok]
    g = _counts.writer_geometry()
    n = g["long_cell"] + 1
    text, said = run_host(host_main, n, ([0, n - 1, 2 * n - 1], list(range(n - 1)) + list(range(n)), [7] * (2 * n - 1)), [0], np.zeros(n, np.int32), 1, cap=g["tile_bytes"] - 1,
                          chunk=g["min_chunk"] + 1)
    assert said["long"] == [1, n] and said["chunk"] == [g["min_chunk"] + 16] and len(text) > g["tile_bytes"]
