"""The Matrix Market writer and the remap of count matrices on the MI355X (include/nabo_counts.h), held byte for byte
to the plain restatement (tests/_counts_ref.py), to what the reference wrote (tests/golden/counts.npz) and to the reader:
read_mtx(write_mtx(M)) gives M back.  The shapes are the smallest at which each path can break: every digit boundary of
values, genes and cells; empty cells first, last and in runs, with the blank-line flag on and off; cells around the
length pass's long-cell threshold; texts built from the geometry the library reports so that a line straddles -- or ends
on -- every chunk and tile boundary; reads of 1, 7, tile - 1 and all bytes; a million entries in more than a dozen
chunks.  The remap: identity, sorted and skipped-sort paths, drops, repeats, the sort's bit counts, a duplicate's lowest
pair, float32 bits.  The file-level functions run under the interpreter that has h5py (tests/_counts_case.py)."""
import io
import json
import os
import re
import subprocess

import numpy as np
import pytest

import _counts_ref as cref
import _ingest_ref as iref
from test_counts_cpu import COMMENT, build_counts_check, golden_matrix
from test_mapping import _interpreter

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def gold(golden):
    return golden("counts")


@pytest.fixture(scope="module")
def ingest(golden):
    return golden("ingest")


@pytest.fixture(scope="module")
def geo(gpu_lib):
    from nabo_amd import _counts
    return _counts.writer_geometry()


def text_of(lib, n_genes, csr, comments=None, blank=False, chunk=0, cap=1 << 24):
    """the whole text through the handle, read cap bytes at a time: (bytes, chunks formatted)"""
    with lib.MtxWriter(csr, n_genes, comments, blank, chunk_bytes=chunk) as w:
        pieces = []
        while True:
            p = w.read(cap)
            if not p:
                break
            assert len(p) == cap or sum(map(len, pieces)) + len(p) == w.total_bytes        # short only at the end
            pieces.append(p)
        text = b"".join(pieces)
        assert len(text) == w.total_bytes and w.read(5) == b""
        return text, w.last_device_ms()[1]


def csr_of(cells, dtype=np.uint32):
    """(cell_ptr, gene, val) of a list of cells, each a list of (gene, value)"""
    return cref.index_of(cells, dtype)


def same(a, b):
    return all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(a, b))


def reads_back(lib, text, n_genes, csr):
    m = lib.read_mtx(io.BytesIO(text))
    return m.n_genes == n_genes and same((m.cell_ptr, m.gene, m.val), csr)


# ---- the writer -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("s", ["A", "B"])
def test_golden_text_equals_the_reference_and_reads_back(gpu_lib, gold, ingest, s):
    n_genes, csr, csc, _, _ = golden_matrix(ingest, s)
    want = gold[s + "_mtx_file_matrix.mtx"].tobytes()
    for chunk in (0, 64, 4096):
        text, _ = text_of(gpu_lib, n_genes, csr, COMMENT, True, chunk)
        assert text == want == cref.mtx_text(n_genes, *csr, COMMENT, blank=True), chunk
    plain, _ = text_of(gpu_lib, n_genes, csr, None, False)
    assert plain == cref.mtx_text(n_genes, *csr) and b"\n\n" not in plain
    for t in (want, plain):
        m = gpu_lib.read_mtx(io.BytesIO(t))
        assert same((m.cell_ptr, m.gene, m.val), csr) and same((m.gene_ptr, m.cell, m.gene_val), csc)
    # a CountMatrix goes in as it came out, and the same call twice gives the same bytes
    out = io.BytesIO()
    assert gpu_lib.write_mtx(m, out, comments=COMMENT, blank_line_for_empty_cell=True) == len(want) and out.getvalue() == want


EDGES = sorted({0, 2 ** 32 - 1} | {10 ** k + d for k in range(1, 10) for d in (-1, 0)})     # 0, 9, 10, 99, 100, ..., 10^9 - 1, 10^9, 2^32 - 1


@pytest.mark.gpu
def test_values_and_genes_at_every_digit_boundary(gpu_lib):
    assert EDGES[:5] == [0, 9, 10, 99, 100] and EDGES[-3:] == [10 ** 9 - 1, 10 ** 9, 2 ** 32 - 1] and len(EDGES) == 20
    genes = [g - 1 for g in EDGES if 1 <= g <= 2 ** 31 - 1] + [2 ** 31 - 2]                  # gene numbers 9, 10, ..., 10^9, 2^31 - 1
    n_genes = 2 ** 31 - 1
    # every value beside every gene width: cell c pairs gene i with value (i + c) mod 20
    csr = csr_of([[(g, EDGES[(i + c) % len(EDGES)]) for i, g in enumerate(genes)] for c in range(len(EDGES))])
    for blank in (False, True):
        text, _ = text_of(gpu_lib, n_genes, csr, None, blank, 64)
        assert text == cref.mtx_text(n_genes, *csr, blank=blank)
    assert b"\n2147483647 1 " in text and b" 4294967295\n" in text and b" 0\n" in text
    # (read_mtx would allocate a gene pointer of 2^31 entries: the reader's restatement reads the text back instead)
    back = iref.parse(text, 1024)
    rows = np.repeat(np.arange(len(EDGES)), np.diff(csr[0]))
    assert back[0] == n_genes and np.array_equal(back[2], csr[1]) and np.array_equal(back[3], rows) and np.array_equal(back[4], csr[2])


@pytest.mark.gpu
def test_cells_up_to_seven_digits(gpu_lib):
    """Cell numbers 1, 9, 10, 99, ..., 999 999, 10^6, 1 000 001 with almost all cells empty.  Cell numbers of 8 to 10
    digits would need 10^7 and more cells; they rest on the digit routine shared with genes and values, which the test
    above drives through all ten widths."""
    n_cells = 1000001
    with_entries = sorted({c - 1 for c in EDGES if 1 <= c <= n_cells} | {0, n_cells - 1})
    assert len(str(with_entries[-1] + 1)) == 7 and with_entries[:3] == [0, 8, 9] and len(with_entries) == 14
    ptr = np.zeros(n_cells + 1, dtype=np.int64)
    ptr[np.array(with_entries) + 1] = 2
    np.cumsum(ptr, out=ptr)
    gene = np.tile(np.array([3, 12345], np.int32), len(with_entries))
    val = np.arange(2 * len(with_entries), dtype=np.uint32) * 1234567
    for blank in (False, True):
        text, chunks = text_of(gpu_lib, 20000, (ptr, gene, val), b"%c\n", blank, 1 << 16)
        assert text == cref.mtx_text(20000, ptr, gene, val, b"%c\n", blank=blank)
        assert chunks == (16 if blank else 1)                    # a million blank lines are a megabyte of text
    assert reads_back(gpu_lib, text, 20000, (ptr, gene, val))


@pytest.mark.gpu
def test_empty_cells_and_empty_matrices(gpu_lib):
    e, a, b = [], [(0, 1)], [(1, 20), (4, 300)]
    for cells in ([e, a, e, e, b, e], [e, e, e], [a], [e], [a, b], [e, e, a, e, e, e, b], []):
        csr = csr_of(cells)
        for blank in (False, True):
            for comments in (None, b"%\n% two lines\n"):
                text, chunks = text_of(gpu_lib, 5, csr, comments, blank, 64, cap=3)
                assert text == cref.mtx_text(5, *csr, comments or b"", blank=blank), (cells, blank)
                assert (chunks == 0) == (len(csr[1]) == 0 and not (blank and cells))
        assert reads_back(gpu_lib, text, 5, csr)
    # n_cells = 0 and nnz = 0: the text is the head alone
    assert text_of(gpu_lib, 7, csr_of([]))[0] == cref.BANNER + b"7 0 0\n"
    assert text_of(gpu_lib, 0, csr_of([e, e]), None, True)[0] == cref.BANNER + b"0 2 0\n\n\n"
    # 20 000 blank lines: more than two tiles of nothing else, and entries behind them
    csr = csr_of([e] * 20000 + [b] + [e] * 3)
    text, _ = text_of(gpu_lib, 5, csr, None, True)
    assert text == cref.mtx_text(5, *csr, blank=True) and reads_back(gpu_lib, text, 5, csr)


@pytest.mark.gpu
def test_long_cells(gpu_lib, geo):
    """A cell of 5 000 entries is longer than the 16 lanes of a group handle in one step, longer than long_cell (it takes the
    workgroup path of the length pass) and its text is longer than one tile; cells of exactly long_cell and long_cell + 1
    entries stand on either side of the threshold."""
    L, T = geo["long_cell"], geo["tile_bytes"]
    rng = np.random.default_rng(7)

    def cell(n, n_genes=60000):
        g = np.sort(rng.choice(n_genes, size=n, replace=False))
        return list(zip(g.tolist(), rng.integers(0, 2 ** 32, size=n).tolist()))
    cells = [cell(3), cell(5000), [], cell(L), cell(L + 1), cell(17), cell(16), cell(15), cell(1), cell(2 * L + 77)]
    csr = csr_of(cells)
    assert L < 5000 and len(cref.mtx_text(60000, *csr_of([cells[1]]))) > T
    for blank, chunk in ((False, 0), (True, 64), (True, T + 64)):
        text, _ = text_of(gpu_lib, 60000, csr, None, blank, chunk)
        assert text == cref.mtx_text(60000, *csr, blank=blank), (blank, chunk)
    assert reads_back(gpu_lib, text, 60000, csr)


def boundary_text(step, n_bytes, on_boundary):
    """Cells of entries whose lines, by the number of digits of their values, either never start on a multiple of `step`
    bytes of the body (a line straddles every such boundary) or start on every one of them: (cells, the body's line
    starts).  Two blank-line cells are mixed in."""
    cells, starts, pos, c = [[]], [], 0, 0
    while pos < n_bytes:
        if len(cells[c]) == 40 or (not cells[c] and c % 7 == 3 and (pos + 1) % step not in (0, 1)):
            if not cells[c]:
                starts.append(pos)                               # a blank line
                pos += 1
            cells.append([])
            c += 1
            continue
        g = len(cells[c]) * 23
        base = len("%d %d " % (g + 1, c + 1)) + 1               # without the value's digits
        room = step - pos % step
        if on_boundary:
            d = room - base if base + 1 <= room <= base + 10 else 1
        else:
            d = 2 if (pos + base + 1) % step == 0 else 1
        starts.append(pos)
        pos += base + d
        cells[c].append((g, min(10 ** d - 1, 2 ** 32 - 1) - (g % 7 if d > 1 else g % 9)))
    if not cells[-1]:
        cells.pop()
    assert len(cells) < 100                                     # (two digits for the cell: `base` stays below 10, so a line always fits in front of a boundary)
    return cells, starts


@pytest.mark.gpu
def test_lines_at_every_chunk_and_tile_boundary(gpu_lib, geo):
    T, C = geo["tile_bytes"], geo["min_chunk"]
    assert T % C == 0
    for on_boundary in (False, True):
        cells, starts = boundary_text(C, 2 * T + 1000, on_boundary)
        csr = csr_of(cells)
        want = cref.mtx_text(1000, *csr, blank=True)
        head = len(cref.BANNER) + len(b"1000 %d %d\n" % (len(cells), len(csr[1])))
        body = want[head:]
        assert [i for i in range(len(body)) if i == 0 or body[i - 1:i] == b"\n"] == starts       # the construction is what the text is
        at = set(starts)
        bounds = range(C, len(body), C)
        if on_boundary:
            assert all(x in at for x in bounds) and T in at and 2 * T in at
        else:
            assert not any(x in at for x in bounds) and len(body) > 2 * T
        assert any(not c for c in cells[:-1])                   # blank lines among them
        # the smallest chunk: a boundary every C bytes; chunks of several tiles: the tile boundaries inside a chunk; one chunk
        for chunk, cap in ((C, 1 << 20), (2 * T + C, T - 1), (0, 7)):
            text, chunks = text_of(gpu_lib, 1000, csr, None, True, chunk, cap)
            assert text == want, (on_boundary, chunk)
            assert chunks == -(-len(body) // (chunk or 1 << 26))
        assert reads_back(gpu_lib, text, 1000, csr)


@pytest.mark.gpu
def test_any_cap(gpu_lib, gold, ingest, geo):
    n_genes, csr, _, _, _ = golden_matrix(ingest, "A")
    want = gold["A_mtx_file_matrix.mtx"].tobytes()
    assert len(want) > 4 * geo["tile_bytes"]
    for cap in (1, 7, geo["tile_bytes"] - 1, len(want), len(want) + 1):
        for chunk in ((4096,) if cap == 1 else (64, 0)):
            assert text_of(gpu_lib, n_genes, csr, COMMENT, True, chunk, cap)[0] == want, (cap, chunk)
    from nabo_amd import _lib
    with gpu_lib.MtxWriter(csr, n_genes) as w:
        buf, n = np.zeros(8, np.uint8), _lib.C.c_int64()
        assert _lib.lib().nabo_mtxw_read(w._h, buf.ctypes.data, 0, _lib.C.byref(n)) == _lib.E_INVALID
        assert _lib.lib().nabo_mtxw_read(w._h, None, 8, _lib.C.byref(n)) == _lib.E_INVALID
        assert w.read(8) == cref.BANNER[:8]
    with pytest.raises(gpu_lib.NaboError) as e:
        gpu_lib.MtxWriter(csr, n_genes, mem_budget=1000)
    assert "error %d:" % _lib.E_NOMEM in str(e.value) and "budget is 1000" in str(e.value)
    with pytest.raises(gpu_lib.NaboError):
        gpu_lib.MtxWriter(csr, n_genes, device=99)


@pytest.fixture(scope="module")
def million():
    """10^6 entries over 70 000 genes x 3 000 cells: (n_genes, csr, csc, the text by Python's %d)"""
    n_genes, n_cells, n = 70000, 3000, 1000000
    rng = np.random.default_rng(2025)
    flat = np.unique(rng.integers(0, n_genes * n_cells, size=n + n // 50))
    flat = np.sort(rng.permutation(flat)[:n])
    gene, cell, val = flat % n_genes, flat // n_genes, rng.integers(0, 2 ** 32, size=n)
    val[::3] %= 100
    csr, csc = iref.index_by(cell, gene, val, n_cells), iref.index_by(gene, cell, val, n_genes)
    return n_genes, csr, csc, iref.mtx_text(n_genes, n_cells, csr[1], cell, csr[2], comments=())


@pytest.mark.gpu
def test_a_million_entries_in_many_chunks(gpu_lib, geo, million):
    n_genes, csr, csc, want = million
    with gpu_lib.MtxWriter(csr, n_genes, chunk_bytes=1 << 20) as w:
        assert w.total_bytes == len(want)
        text = b"".join(iter(lambda: w.read(3 << 20), b""))
        ms, chunks = w.last_device_ms()
    assert text == want and chunks > 12 and chunks == -(-(len(want) - want.index(b"\n", 50) - 1) // (1 << 20))
    assert set(ms) == {"upload", "lengths", "format", "download"} and all(v > 0 for v in ms.values())
    # the same call again, and the default chunk (one piece, some two thousand tiles)
    again, _ = text_of(gpu_lib, n_genes, csr, None, False, 1 << 20)
    whole, one = text_of(gpu_lib, n_genes, csr)
    assert again == text and whole == text and one == 1
    m = gpu_lib.read_mtx(io.BytesIO(text))
    assert same((m.cell_ptr, m.gene, m.val), csr) and same((m.gene_ptr, m.cell, m.gene_val), csc)


@pytest.mark.gpu
def test_plain_c_consumer(gpu_lib, gold, ingest, tmp_path):
    exe = build_counts_check(tmp_path)
    n_genes, csr, _, _, _ = golden_matrix(ingest, "B")
    blob = np.array([n_genes, len(csr[0]) - 1], np.int64).tobytes() + csr[0].tobytes() + csr[1].tobytes() + csr[2].tobytes()
    for cap, blank in ((1000, 1), (5, 0)):
        r = subprocess.run([exe, "run", str(cap), str(blank)], input=blob, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:]
        assert r.stdout == cref.mtx_text(n_genes, *csr, b"% plain C\n", blank=bool(blank))
    bad = blob[:16] + np.array(csr[0][::-1]).tobytes() + blob[16 + csr[0].nbytes:]
    r = subprocess.run([exe, "run", "100", "0"], input=bad, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert r.returncode == 1 and r.stdout.startswith(b"error -1: cell_ptr")


# ---- the remap --------------------------------------------------------------------------------------------------------
def random_matrix(rng, n_rows, n_cols, most, dtype=np.uint32):
    rows = []
    for _ in range(n_rows):
        n = int(rng.integers(0, most + 1))
        idx = np.sort(rng.choice(n_cols, size=min(n, n_cols), replace=False))
        rows.append(list(zip(idx.tolist(), rng.integers(0, 2 ** 32, size=len(idx)).tolist())))
    return csr_of(rows, dtype)


def remap_agrees(lib, m, n_cols, row_src, col_map, n_out_cols):
    got = lib.remap_counts(m[0], m[1], m[2], n_cols, row_src, col_map, n_out_cols)
    want = cref.remap(m[0], m[1], m[2], row_src, col_map, n_out_cols)
    for g, w in zip(got, want):
        assert g[0].dtype == np.int64 and g[1].dtype == np.int32 and g[2].dtype == m[2].dtype
        assert np.array_equal(g[0], w[0]) and np.array_equal(g[1], w[1]) and g[2].tobytes() == w[2].tobytes(), (n_cols, n_out_cols)
    only = lib.remap_counts(m[0], m[1], m[2], n_cols, row_src, col_map, n_out_cols, with_csc=False)
    assert only[1] is None and all(a.tobytes() == b.tobytes() for a, b in zip(only[0], got[0]))     # (bytes: a NaN payload is not equal to itself)
    return got


@pytest.mark.gpu
def test_remap_identity_returns_the_input(gpu_lib, ingest):
    n_genes, csr, csc, _, _ = golden_matrix(ingest, "A")
    got = gpu_lib.remap_counts(*csr, n_genes, np.arange(300), np.arange(n_genes), n_genes)
    assert all(a.tobytes() == b.tobytes() and a.dtype == b.dtype for a, b in zip(got[0], csr))
    assert all(a.tobytes() == b.tobytes() and a.dtype == b.dtype for a, b in zip(got[1], csc))
    # the CSC is the transpose the reader's stage gives on its own
    f = (csr[2] % 1000).astype(np.float32)
    t = gpu_lib.csr_to_csc(csr[0], csr[1], f, n_genes)
    r = gpu_lib.remap_counts(csr[0], csr[1], f, n_genes, np.arange(300), np.arange(n_genes), n_genes)[1]
    assert all(np.array_equal(a, b) and a.dtype == b.dtype for a, b in zip(r, t))
    sub = gpu_lib.subset_cells(gpu_lib.read_mtx(io.BytesIO(cref.mtx_text(n_genes, *csr))), [5, 299, 5, 0])
    want = cref.subset(*csr, n_genes, [5, 299, 5, 0])
    assert same((sub.cell_ptr, sub.gene, sub.val), want[0]) and same((sub.gene_ptr, sub.cell, sub.gene_val), want[1]) and sub.n_cells == 4


@pytest.mark.gpu
def test_remap_sorted_and_skipped_sort_paths(gpu_lib):
    rng = np.random.default_rng(11)
    m = random_matrix(rng, 70, 50, 30)
    rows = rng.integers(0, 70, size=90)                          # repeats; some rows never taken
    shuffled = rng.permutation(50).astype(np.int32)
    rising = np.arange(50, dtype=np.int32)
    for col_map in (shuffled, rising):
        dropped = col_map.copy()
        dropped[rng.choice(50, size=12, replace=False)] = -1
        for cm in (col_map, dropped):
            remap_agrees(gpu_lib, m, 50, rows, cm, 50)
    # a rising map onto fewer columns (renumbered), all columns dropped, no rows, empty rows only, no entries at all
    keep = np.sort(rng.choice(50, size=20, replace=False))
    narrow = np.full(50, -1, np.int32)
    narrow[keep] = np.arange(20)
    remap_agrees(gpu_lib, m, 50, rows, narrow, 20)
    got = remap_agrees(gpu_lib, m, 50, rows, np.full(50, -1, np.int32), 7)
    assert got[0][0].tolist() == [0] * 91 and got[1][0].tolist() == [0] * 8 and len(got[0][1]) == 0
    got = remap_agrees(gpu_lib, m, 50, np.zeros(0, np.int64), shuffled, 50)
    assert got[0][0].tolist() == [0] and got[1][0].tolist() == [0] * 51
    empty = np.flatnonzero(np.diff(m[0]) == 0)
    assert len(empty) >= 1
    remap_agrees(gpu_lib, m, 50, np.repeat(empty, 3), shuffled, 50)
    remap_agrees(gpu_lib, csr_of([[], []]), 4, [1, 0, 1], [3, 2, 1, 0], 4)


@pytest.mark.gpu
def test_remap_around_the_sort_bit_counts(gpu_lib):
    """the sort runs over the bits of n_out_cols - 1 and of n_out_rows - 1: one column, 2^k and 2^k + 1 columns (k = 8 and
    16, below and above 16 bits), with the top column in use, and the same for the rows"""
    rng = np.random.default_rng(13)
    m = random_matrix(rng, 40, 300, 25)
    for n_out in (1, 2, 256, 257, 65536, 65537):
        # distinct targets, so no row can hold one twice; the column of the first entry goes to the top column
        take = [int(m[1][0])] + [int(c) for c in rng.permutation(300) if c != m[1][0]][:min(n_out, 200) - 1]
        col_map = np.full(300, -1, np.int32)
        col_map[take] = [n_out - 1] + rng.permutation(n_out - 1)[:len(take) - 1].tolist()
        got = remap_agrees(gpu_lib, m, 300, list(range(40)), col_map, n_out)
        assert int(got[0][1].max()) == n_out - 1 and len(got[0][1]) >= 1
    for n_rows_out in (1, 2, 256, 257):
        remap_agrees(gpu_lib, m, 300, rng.integers(0, 40, size=n_rows_out), rng.permutation(300).astype(np.int32), 300)


@pytest.mark.gpu
def test_remap_a_row_of_5000_entries(gpu_lib):
    rng = np.random.default_rng(17)
    cols = np.sort(rng.choice(6000, size=5000, replace=False))
    m = csr_of([[(3, 1)], list(zip(cols.tolist(), rng.integers(0, 2 ** 32, size=5000).tolist())), [], [(5999, 2)]])
    for col_map in (np.arange(6000)[::-1].astype(np.int32), np.arange(6000, dtype=np.int32), rng.permutation(6000).astype(np.int32)):
        col_map = col_map.copy()
        col_map[::11] = -1
        remap_agrees(gpu_lib, m, 6000, [1, 3, 1, 0, 2], col_map, 6000)


@pytest.mark.gpu
def test_remap_names_the_lowest_duplicate(gpu_lib):
    from nabo_amd import _lib
    m = csr_of([[(0, 1), (1, 2), (2, 3)], [(1, 1), (3, 2)], [(0, 5), (2, 6), (3, 7)], [(4, 9)]])
    cases = [([2, 0, 0, 0, 1], 3, [1, 3, 0, 2]),                # columns 1, 2, 3 -> 0: every row but row 3 holds it twice
             ([1, 0, 1, 0, 2], 3, [3, 2, 0]),                   # the sorted path: 0, 2 -> 1 and 1, 3 -> 0
             ([0, 1, 1, 2, 2], 3, [0, 1, 2, 3])]                # the skipped sort: a map that does not decrease
    for col_map, n_out, rows in cases:
        with pytest.raises(cref.Duplicate) as want:
            cref.remap(*m, rows, col_map, n_out)
        with pytest.raises(ValueError) as e:
            gpu_lib.remap_counts(*m, 5, rows, col_map, n_out)
        got = re.search(r"output row (\d+) holds output column (\d+)", str(e.value))
        assert got and (int(got.group(1)), int(got.group(2))) == (want.value.row, want.value.col), str(e.value)
    # the same columns are no duplicate when no row holds two of them
    remap_agrees(gpu_lib, m, 5, [3, 1], [2, 0, 0, 1, 1], 3)
    one = np.zeros(4, np.int64)
    assert _lib.lib().nabo_counts_remap(99, 0, 0, one.ctypes.data, None, None, 0, None, 0, None, _lib.C.byref(_lib.C.c_int64()), one.ctypes.data, None, None,
                                        None, None, None) == _lib.E_NODEVICE


@pytest.mark.gpu
def test_remap_keeps_float32_bits(gpu_lib):
    rng = np.random.default_rng(19)
    m = random_matrix(rng, 30, 40, 20)
    bits = m[2].copy()
    bits[:6] = [0x7FC00001, 0xFFC00000, 0x80000000, 0x7F800000, 0x00000001, 0xFF800000]      # NaNs with payloads, -0.0, inf, a denormal, -inf
    f = bits.view(np.float32)
    for col_map in (rng.permutation(40).astype(np.int32), np.arange(40, dtype=np.int32)):
        got = remap_agrees(gpu_lib, (m[0], m[1], f), 40, rng.integers(0, 30, size=45), col_map, 40)
        assert got[0][2].dtype == np.float32 and got[1][2].dtype == np.float32


@pytest.mark.gpu
def test_merge_counts_against_the_restatement(gpu_lib):
    rng = np.random.default_rng(23)
    names = ["G%03d" % i for i in range(60)]
    mats, genes, cells = [], [], []
    for k, (n_cells, n_genes) in enumerate(((20, 30), (15, 25), (10, 40))):
        g = [names[i] for i in rng.permutation(60)[:n_genes]]   # different gene sets, in no order
        csr = random_matrix(rng, n_cells, n_genes, 12)
        mats.append(gpu_lib.read_mtx(io.BytesIO(cref.mtx_text(n_genes, *csr))))
        genes.append(g)
        cells.append(["c%d" % i for i in range(n_cells)])
    union = sorted(set(sum(genes, [])))
    assert len(union) > max(map(len, genes))
    merged = [c + "-" + s for k, s in enumerate("abc") for c in cells[k]]
    order = [merged[i] for i in rng.permutation(len(merged))]
    m, g, c = gpu_lib.merge_counts(mats, genes, cells, list("abc"), cell_order=order)
    want = cref.merge([(x.cell_ptr, x.gene, x.val) for x in mats], genes, cells, list("abc"), order)
    assert g == union == want[2] and c == order and (m.n_genes, m.n_cells) == (len(union), 45)
    assert same((m.cell_ptr, m.gene, m.val), want[0]) and same((m.gene_ptr, m.cell, m.gene_val), want[1])
    # the default order: a permutation that the seed alone decides
    m1, _, c1 = gpu_lib.merge_counts(mats, genes, cells, seed=5)
    m2, _, c2 = gpu_lib.merge_counts(mats, genes, cells, seed=5)
    _, _, c3 = gpu_lib.merge_counts(mats, genes, cells, seed=6)
    assert c1 == c2 and c1 != c3 and sorted(c1) == sorted(x + "-" + str(k + 1) for k in range(3) for x in cells[k]) and same((m1.cell_ptr, m1.gene), (m2.cell_ptr, m2.gene))
    with pytest.raises(ValueError):
        gpu_lib.merge_counts(mats, genes, cells, ["a", "b"])
    with pytest.raises(ValueError):
        gpu_lib.merge_counts(mats, genes, cells, cell_order=order)                       # names with the default suffixes are others


# ---- the files --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_file_level_functions(gpu_lib):
    py = _interpreter()
    if py is None:
        pytest.skip("no interpreter with h5py in this image")
    r = subprocess.run([py, os.path.join(HERE, "_counts_case.py")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][len("RESULT "):])
    assert res["checked"] == 27 and res["differ"] == [], res
