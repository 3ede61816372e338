"""The per-cell quality-control sums on the MI355X (nabo_cell_qc, nabo_amd._qc): through the C ABI bit-equal to the
tests' plain restatement, which sums in the header's order (tests/_qc_ref.py), on both golden samples
(tests/golden/qc.npz) in one chunk and in forced chunks; the edges of the kernel's geometry -- groups of 16 lanes, 32
cells per workgroup, the class table in LDS and through L2; 100 001 cells, where every workgroup walks its tile loop
several times; subnormal values; the argument checks of the C entry point; the file-level
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


MANY_CELLS = 100001                     # 3 126 tiles of 32 cells, the last one of a single cell


def cu_count():
    """the number cell_qc.hip's launcher reads: hipDeviceGetAttribute(hipDeviceAttributeMultiprocessorCount, which is 63 in
    hip_runtime_api.h) of device 0, asked of the HIP runtime the library has loaded into this process (torch brings a
    runtime of its own, which sees no device once another one is in use)"""
    import ctypes
    with open("/proc/self/maps") as f:
        loaded = sorted(set(ln.split()[-1] for ln in f if "libamdhip64" in ln and "/torch/" not in ln))
    assert len(loaded) == 1, loaded
    n = ctypes.c_int(0)
    assert ctypes.CDLL(loaded[0]).hipDeviceGetAttribute(ctypes.byref(n), 63, 0) == 0
    assert 8 <= n.value <= 4096, n.value
    return n.value


def many_cells(n_raw, long_at, seed):
    """MANY_CELLS cells over n_raw genes: 0 .. 5 entries each (strictly increasing genes from the lower five eighths of
    the table), every 307th cell 17 .. 200 entries drawn from all genes with gene 0 and gene n_raw - 1 among them, cell
    `long_at` 3 000 entries (n_raw when there are fewer genes), the last cell empty; values with fractions and stored
    zeros as in edge_cells; a random class byte per gene"""
    rng = np.random.default_rng(seed)
    n = MANY_CELLS
    lens = rng.integers(0, 6, n)
    long_cells = np.arange(150, n - 1, 307)
    lens[long_cells] = rng.integers(17, 201, long_cells.shape[0])
    lens[long_at] = min(3000, n_raw)
    lens[n - 1] = 0
    cell_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    gene = np.zeros(int(cell_ptr[-1]), dtype=np.int32)
    few = np.nonzero(lens <= 5)[0]
    g5 = np.cumsum(rng.integers(1, n_raw // 8 + 1, (few.shape[0], 5)), axis=1) - 1       # at most 5 (n_raw // 8) - 1
    inside = np.arange(5)[None, :] < lens[few][:, None]
    gene[(cell_ptr[few][:, None] + np.arange(5)[None, :])[inside]] = g5[inside]
    for c in np.nonzero(lens > 5)[0].tolist():
        g = np.sort(rng.permutation(n_raw)[:lens[c]])
        g[0], g[-1] = 0, n_raw - 1
        gene[cell_ptr[c]:cell_ptr[c + 1]] = g
    val = (rng.poisson(1.5, gene.shape[0]) * rng.random(gene.shape[0])).astype(np.float32)
    return cell_ptr, gene, val, rng.integers(0, 256, n_raw).astype(np.uint8)


@pytest.mark.gpu
@pytest.mark.parametrize("n_classes,n_raw", [(0, 5000), (3, 5000), (2, 65537), (8, 65536), (5, 70000), (7, 600)])
def test_more_tiles_than_workgroups(gpu_lib, n_classes, n_raw):
    """100 001 cells: every workgroup walks its tile loop several times, and not all the same number of times.
    (0, 5000): the kernel without classes; (3, 5000): <3, true>, the table in LDS; (2, 65537): <3, false>, the table
    through L2; (8, 65536): <8, true> with the 64 KiB table, two workgroups per CU and the attribute call, so twice the
    trips; (5, 70000): <8, false> and (7, 600): <8, true>, both with fewer output columns than the nine accumulators
    (the store guard and the bit mask below 8).  The 3 000-entry cell sits in a tile of the second trip.  Bit-equal to
    the header's order (n_entries too), two runs alike, and alike in three or more chunks."""
    from nabo_amd import _qc
    cus = cu_count()
    n_tiles = -(-MANY_CELLS // 32)
    assert n_tiles > 2 * 4 * cus, "a device of %d CUs walks %d tiles in two trips or fewer: this test needs more cells" % (cus, n_tiles)
    # cell_qc.hip's grid: CUs x min(4, 160 KiB / the table's bytes in LDS) workgroups
    table = -(-n_raw // 16) * 16 if 0 < n_classes and n_raw <= _qc.LDS_TABLE_GENES else 0
    grid = cus * (min(4, 160 * 1024 // table) if table else 4)
    print("%d CUs, %d workgroups, %d tiles: %d or %d trips per workgroup" % (cus, grid, n_tiles, n_tiles // grid, -(-n_tiles // grid)))
    assert n_tiles // grid >= 2 and n_tiles % grid != 0        # every workgroup loops, and not all equally often
    long_at = (grid + 5) * 32 + 9
    cell_ptr, gene, val, cls = many_cells(n_raw, long_at, seed=n_raw + n_classes)
    lens = np.diff(cell_ptr)
    assert lens[long_at] == min(3000, n_raw) and lens[-1] == 0 and gene.min() == 0 and gene.max() == n_raw - 1
    assert ((lens > 16) & (lens <= 200)).sum() > 300 and (lens <= 5).sum() > 99000
    want = qref.cell_qc_many(cell_ptr, gene, val, cls, n_classes)
    assert np.array_equal(want[0], lens)
    kw = dict(gene_class=cls, n_classes=n_classes)
    got = gpu_lib.cell_qc_csr(cell_ptr, gene, val, **kw)
    assert _qc.last_device_ms()[1] == 1
    differ = np.nonzero((_bits(got[1]) != _bits(want[1])).any(axis=1) | (got[0] != want[0]))[0]
    assert got[1].shape == (MANY_CELLS, 1 + n_classes) and _same(got, want), (differ[:8].tolist(), (differ[:8] // 32).tolist())
    assert _same(gpu_lib.cell_qc_csr(cell_ptr, gene, val, **kw), got)
    budget = int(8 * gene.shape[0] + (16 + 8 * (1 + n_classes)) * MANY_CELLS) // 3
    chunked = gpu_lib.cell_qc_csr(cell_ptr, gene, val, mem_budget=budget, **kw)
    assert _qc.last_device_ms()[1] >= 3 and _same(chunked, got)


@pytest.mark.gpu
def test_subnormal_values_are_summed_not_flushed(gpu_lib):
    """float32 values below 2^-126 (1e-40, the smallest subnormal, some around ordinary values): the float64 sums are
    the restatement's bit for bit, so the conversion to float64 keeps them"""
    tiny = np.float32(1e-40)
    assert 0 < tiny < np.finfo(np.float32).tiny
    rng = np.random.default_rng(11)
    lengths = [3, 16, 17, 70, 0, 5]
    cell_ptr, gene, val, cls = edge_cells(300, lengths, seed=12)
    val[:] = (tiny * rng.integers(1, 100, val.shape[0])).astype(np.float32)
    val[cell_ptr[1]] = np.float32(1.401298464324817e-45)         # the smallest subnormal
    val[cell_ptr[3]:cell_ptr[4]:3] = np.float32(0.375)           # cell 3: ordinary values among them
    val[cell_ptr[5]:cell_ptr[6]] = [1e-38, 1e-39, 0.0, 2e-45, 1.17549435e-38]
    assert ((val > 0) & (val < np.finfo(np.float32).tiny)).sum() > 80
    for n_classes in (0, 3, 8):
        want = qref.cell_qc(cell_ptr, gene, val, cls if n_classes else None, n_classes)
        got = gpu_lib.cell_qc_csr(cell_ptr, gene, val, gene_class=cls, n_classes=n_classes)
        assert _same(got, want), n_classes
        assert (want[1][[0, 1, 2, 5], 0] > 0).all() and (want[1][[0, 1, 2], 0] < 1e-34).all()


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
