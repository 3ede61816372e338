"""The per-cell quality-control sums on the MI355X (nabo_cell_qc, nabo_amd._qc): through the C ABI bit-equal to the
tests' plain restatement, which sums in the header's order (tests/_qc_ref.py), on both golden samples
(tests/golden/qc.npz) in one chunk and in forced chunks; the edges of the kernel's geometry -- groups of 16 lanes, 32
cells per workgroup, the class table in LDS and through L2; the argument checks of the C entry point; the file-level
functions on files written from the golden; and the plain-C consumer."""
import json
import os
import subprocess

import numpy as np
import pytest

import _qc_ref as qref
from test_mapping import _interpreter
from test_qc_cpu import build_qc_check

HERE = os.path.dirname(os.path.abspath(__file__))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same(got, want):
    return (got[0].dtype == np.int64 and np.array_equal(got[0], want[0]) and got[1].shape == want[1].shape
            and np.array_equal(_bits(got[1]), _bits(want[1])))


@pytest.fixture(scope="module")
def gold(golden):
    return golden("qc")


@pytest.fixture(scope="module")
def restated(gold):
    """the restatement of both samples with three classes (mito, ribo, the reference's kept genes), computed once"""
    out = {}
    for s in ("A", "B"):
        cls = qref.class_bits(gold["genes"], *qref.patterns_of(gold), keep_genes=gold[s + "_keep_genes"])
        out[s] = (cls, qref.cell_qc(gold["cell_ptr"], gold["gene"], gold[s + "_val"], cls, 3))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("s", ["A", "B"])
def test_golden_samples_bit_equal_to_the_restatement(gpu_lib, gold, restated, s):
    """integer counts (A) and non-integer values (B): the device's sums are the header's order bit for bit, whole and
    in chunks; float32 of sample A's sums are the reference's float32 sums"""
    from nabo_amd import _qc
    m = (gold["cell_ptr"], gold["gene"], gold[s + "_val"])
    cls, want = restated[s]
    got = gpu_lib.cell_qc_csr(*m, gene_class=cls, n_classes=3)
    ms, chunks = _qc.last_device_ms()
    print("sample %s: %d chunks, device ms %s" % (s, chunks, ms))
    assert chunks == 1 and _same(got, want)
    chunked = gpu_lib.cell_qc_csr(*m, gene_class=cls, n_classes=3, mem_budget=40000)
    assert _qc.last_device_ms()[1] > 4 and _same(chunked, want)
    ref = np.stack([gold[s + "_tot"], gold[s + "_cum_mito"], gold[s + "_cum_ribo"]], axis=1)
    assert np.array_equal(got[0], gold[s + "_ngenes"].astype(np.int64))
    if s == "A":
        assert np.array_equal(got[1][:, :3].astype(np.float32), ref)
    else:
        rel = (np.abs(got[1][:, :3] - ref)[ref != 0] / ref[ref != 0]).max()
        print("sample B: deviation from the reference's float32 sums %.3g (measured %.3g)" % (rel, float(gold["tot_dev"])))
        assert rel <= 4 * float(gold["tot_dev"])
    # fewer classes than the table holds bits: the higher bits are ignored
    two = gpu_lib.cell_qc_csr(*m, gene_class=cls, n_classes=2)
    assert _same(two, (want[0], want[1][:, :3]))
    with pytest.raises(gpu_lib.NaboError) as e:
        gpu_lib.cell_qc_csr(*m, gene_class=cls, n_classes=3, mem_budget=64)
    assert "budget" in str(e.value)


def edge_cells(n_raw, lengths, seed):
    """cells of the given lengths over n_raw genes; gene 0 and gene n_raw - 1 are listed wherever a cell has room; values
    with fractions, stored zeros among them; a random class byte per gene"""
    rng = np.random.default_rng(seed)
    rows = []
    for n in lengths:
        n = min(n, n_raw)
        g = np.sort(rng.permutation(n_raw)[:n])
        if n >= 2:
            g[0], g[-1] = 0, n_raw - 1
        rows.append(g)
    cell_ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    gene = np.concatenate(rows + [np.zeros(0, np.int64)]).astype(np.int32)
    val = (rng.poisson(1.5, gene.shape[0]) * rng.random(gene.shape[0])).astype(np.float32)
    return cell_ptr, gene, val, rng.integers(0, 256, n_raw).astype(np.uint8)


EDGE_LENGTHS = [0, 1, 15, 16, 17, 63, 64, 65, 3000, 0, 2, 129, 4097]


@pytest.mark.gpu
@pytest.mark.parametrize("n_raw,n_classes,n_cells", [(5000, 8, 13), (5000, 0, 13), (5000, 3, 13), (5000, 1, 1), (5000, 8, 33), (1, 8, 7),
                                                     (1, 0, 1), (65536, 8, 13), (65537, 8, 300), (65537, 2, 33)])
def test_edges_of_the_geometry(gpu_lib, n_raw, n_classes, n_cells):
    """cells of 0, 1, 15 .. 17, 63 .. 65 and a few thousand entries in one call; one cell; one cell more than a workgroup
    holds; one raw gene; no class and eight; the first and the last gene; a table of 65536 genes (LDS) and of 65537
    (through L2); rows repeated and out of order; chunks that end between two short cells; two runs bit-equal"""
    from nabo_amd import _qc
    assert _qc.LDS_TABLE_GENES == 65536
    lengths = (EDGE_LENGTHS * (n_cells // len(EDGE_LENGTHS) + 1))[:n_cells]
    cell_ptr, gene, val, cls = edge_cells(n_raw, lengths, seed=n_raw + n_classes + n_cells)
    if n_classes == 0:
        cls = None
    want = qref.cell_qc(cell_ptr, gene, val, cls, n_classes)
    kw = dict(gene_class=cls if cls is not None else np.zeros(n_raw, np.uint8), n_classes=n_classes)
    got = gpu_lib.cell_qc_csr(cell_ptr, gene, val, **kw)
    assert got[1].shape == (n_cells, 1 + n_classes) and _same(got, want)
    assert _same(gpu_lib.cell_qc_csr(cell_ptr, gene, val, **kw), got)
    rows = np.concatenate([np.arange(n_cells)[::-1], [0, 0, n_cells - 1], np.arange(n_cells)[:5]])
    assert _same(gpu_lib.cell_qc_csr(cell_ptr, gene, val, rows=rows, **kw), (want[0][rows], want[1][rows]))
    # 8 bytes per entry and 16 + 8 (1 + n_classes) per row: the longest cell alone fills a chunk, the short cells before
    # and after it share others
    budget = int(8 * np.diff(cell_ptr).max() + 16 + 8 * (1 + n_classes))
    chunked = gpu_lib.cell_qc_csr(cell_ptr, gene, val, rows=rows, mem_budget=budget, **kw)
    assert _same(chunked, (want[0][rows], want[1][rows]))
    if n_cells > 8:
        assert _qc.last_device_ms()[1] >= 3
    empty = gpu_lib.cell_qc_csr(cell_ptr, gene, val, rows=np.zeros(0, np.int64), **kw)
    assert empty[0].shape == (0,) and empty[1].shape == (0, 1 + n_classes)


@pytest.mark.gpu
def test_a_sum_float32_gets_wrong(gpu_lib):
    """16777216 + 1 + 1 in one cell, in every order across the 16 partial sums' lanes"""
    cls = np.array([1, 0, 1, 1] + [0] * 30, np.uint8)
    for genes, vals in (([0, 1, 2], [16777216.0, 1.0, 1.0]), ([0, 1, 2], [1.0, 1.0, 16777216.0]),
                        (list(range(17)), [16777216.0] + [0.0] * 15 + [1.0]), (list(range(34)), [1.0] * 33 + [16777216.0])):
        n, s = gpu_lib.cell_qc_csr([0, len(genes)], genes, vals, gene_class=cls, n_classes=1)
        member = cls[genes].astype(bool)
        assert n.tolist() == [len(genes)] and s.tolist() == [[float(np.sum(vals, dtype=np.float64)), float(np.sum(np.array(vals)[member], dtype=np.float64))]]
        assert s[0, 0] != float(np.float32(16777216.0) + np.float32(1.0))


@pytest.mark.gpu
def test_the_c_entry_point_refuses_bad_arguments(gpu_lib):
    """every NABO_E_INVALID case of nabo_cell_qc, past the Python wrapper's own checks"""
    from nabo_amd import _qc
    i64, i32, f32, u8 = np.int64, np.int32, np.float32, np.uint8
    good = dict(cell_ptr=np.array([0, 2, 3], i64), gene=np.array([0, 2, 1], i32), val=np.array([1, 2, 3], f32), gene_class=np.array([1, 0, 3], u8),
                n_classes=2, rows=None)
    assert _qc._device_qc(**good)[1].tolist() == [[3.0, 3.0, 2.0], [3.0, 0.0, 0.0]]
    for change, word in (({"cell_ptr": np.array([1, 2, 3], i64)}, "cell_ptr[0]"), ({"cell_ptr": np.array([0, 3, 2], i64)}, "monotone"),
                         ({"gene": np.array([0, 3, 1], i32)}, "not a gene"), ({"gene": np.array([0, -1, 1], i32)}, "not a gene"),
                         ({"gene": np.array([2, 0, 1], i32)}, "strictly increasing"), ({"gene": np.array([1, 1, 0], i32)}, "strictly increasing"),
                         ({"val": np.array([1, np.nan, 3], f32)}, "finite"), ({"val": np.array([1, np.inf, 3], f32)}, "finite"),
                         ({"val": np.array([1, -2, 3], f32)}, "finite"), ({"n_classes": 9}, "n_classes"), ({"n_classes": -1}, "n_classes"),
                         ({"rows": np.array([0, 2], i64)}, "rows[1]"), ({"rows": np.array([-1], i64)}, "rows[0]")):
        with pytest.raises(ValueError) as e:
            _qc._device_qc(**dict(good, **change))
        assert word in str(e.value), (change, str(e.value))
    L = _qc._lib.lib()
    out_n, out_s = np.zeros(2, i64), np.zeros(6)
    a = [good[k].ctypes.data for k in ("cell_ptr", "gene", "val")]
    assert L.nabo_cell_qc(0, 2, 3, None, a[1], a[2], 2, good["gene_class"].ctypes.data, 0, None, 0, out_n.ctypes.data, out_s.ctypes.data) == _qc._lib.E_INVALID
    assert L.nabo_cell_qc(0, 2, 3, a[0], None, a[2], 2, good["gene_class"].ctypes.data, 0, None, 0, out_n.ctypes.data, out_s.ctypes.data) == _qc._lib.E_INVALID
    assert L.nabo_cell_qc(0, 2, 3, a[0], a[1], a[2], 2, None, 0, None, 0, out_n.ctypes.data, out_s.ctypes.data) == _qc._lib.E_INVALID
    assert L.nabo_cell_qc(0, 2, 3, a[0], a[1], a[2], 2, good["gene_class"].ctypes.data, 0, None, 0, None, out_s.ctypes.data) == _qc._lib.E_INVALID
    assert L.nabo_cell_qc(0, 2, 3, a[0], a[1], a[2], 2, good["gene_class"].ctypes.data, 0, None, 0, out_n.ctypes.data, None) == _qc._lib.E_INVALID
    assert L.nabo_cell_qc(0, -1, 3, a[0], a[1], a[2], 2, good["gene_class"].ctypes.data, 0, None, 0, out_n.ctypes.data, out_s.ctypes.data) == _qc._lib.E_INVALID
    assert L.nabo_cell_qc(99, 2, 3, a[0], a[1], a[2], 2, good["gene_class"].ctypes.data, 0, None, 0, out_n.ctypes.data, out_s.ctypes.data) == _qc._lib.E_NODEVICE


@pytest.mark.gpu
def test_file_level_functions_through_to_the_pca(gpu_lib):
    py = _interpreter()
    if py is None:
        pytest.skip("no interpreter with h5py in this image")
    r = subprocess.run([py, os.path.join(HERE, "_qc_case.py")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][len("RESULT "):])
    assert res["checked"] == 37 and res["differ"] == [], res


@pytest.mark.gpu
def test_plain_c_consumer_reproduces_a_golden_call(gpu_lib, gold, restated, tmp_path):
    exe = build_qc_check(tmp_path)
    cls, want = restated["B"]
    rows = np.arange(len(gold["cells"]))[::-1][:60]
    ptr, gene, val = gold["cell_ptr"], gold["gene"], gold["B_val"]
    text = "%d %d 3 %d\n" % (len(ptr) - 1, len(cls), len(rows)) + " ".join(str(int(x)) for x in ptr) + "\n"
    text += "\n".join("%d %r" % (int(g), float(v)) for g, v in zip(gene, val)) + "\n" + " ".join(str(int(x)) for x in cls) + "\n"
    text += " ".join(str(int(x)) for x in rows) + "\n"
    r = subprocess.run([exe, "run"], input=text, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
    assert r.returncode == 0, r.stdout
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("row ")]
    got = (np.array([int(w[2]) for w in lines], dtype=np.int64), np.array([[float(x) for x in w[3:]] for w in lines]))
    assert _same(got, (want[0][rows], want[1][rows]))
