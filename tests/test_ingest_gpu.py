"""The Matrix Market reader on the MI355X (include/nabo_ingest.h), through the C ABI and read_mtx, held byte for byte to
the plain restatement (tests/_ingest_ref.py) and to what the reference wrote (tests/golden/ingest.npz): both golden
directories at several chunk sizes and splits; the edges of the kernel's geometry, built from nabo_mtx_geometry; the
grammar, case by case; the lowest bad line; order independence; a million entries in more than a dozen chunks with
70 000 genes; repeatability; the transpose on its own; the chain into the QC and statistics entry points; the file-level
mtx_to_h5; and a plain-C consumer.  Errors are compared by status and line, never by message text.

The parse kernel's grid is one workgroup per tile and no workgroup loops over tiles, so there is no case of a chunk with
more tiles than workgroups; the million-entry case has chunks of 64 tiles and the golden cases chunks of less than one."""
import ctypes as C
import gzip
import io
import json
import os
import re
import subprocess

import numpy as np
import pytest

import _ingest_ref as iref
import _qc_ref as qref
from test_ingest_cpu import HEAD, LINES, build_ingest_check, files_of, mtx_bytes, reference_indexes, same_index, write_dir
from test_mapping import _interpreter

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def gold(golden):
    return golden("ingest")


@pytest.fixture(scope="module")
def geo(gpu_lib):
    from nabo_amd import _ingest
    return _ingest.geometry()


def run_abi(data, chunk=0, split=0):
    """the file through the C ABI, `split` bytes per feed (0: all at once): (0, None, CountMatrix) or (status, line, None)"""
    from nabo_amd import _ingest, _lib
    L = _lib.lib()

    def failed(rc):
        m = re.match(r"line (\d+):", L.nabo_last_error().decode())
        return rc, int(m.group(1)) if m else None, None

    r = _ingest.MtxReader(chunk_bytes=chunk)
    try:
        step = split if split > 0 else max(len(data), 1)
        for at in range(0, len(data), step):
            piece = data[at:at + step]
            rc = L.nabo_mtx_feed(r._h, piece, len(piece))
            if rc:
                return failed(rc)
        ng, nc, nnz = C.c_int64(), C.c_int64(), C.c_int64()
        rc = L.nabo_mtx_finish(r._h, C.byref(ng), C.byref(nc), C.byref(nnz))
        if rc:
            return failed(rc)
        # (finish() of the wrapper would call nabo_mtx_finish again: fetch the arrays here)
        ng, nc, nnz = int(ng.value), int(nc.value), int(nnz.value)
        a = [np.zeros(nc + 1, np.int64), np.zeros(nnz, np.int32), np.zeros(nnz, np.uint32), np.zeros(ng + 1, np.int64), np.zeros(nnz, np.int32),
             np.zeros(nnz, np.uint32)]
        p = [x.ctypes.data if x.size else None for x in a]
        assert L.nabo_mtx_get_csr(r._h, p[0], p[1], p[2]) == 0 and L.nabo_mtx_get_csc(r._h, p[3], p[4], p[5]) == 0
        return 0, None, _ingest.CountMatrix(ng, nc, *a)
    finally:
        r.close()


def indexes(m):
    return (m.cell_ptr, m.gene, m.val), (m.gene_ptr, m.cell, m.gene_val)


def agrees(data, max_line, chunk=0, split=0):
    """the library against the restatement on one file: the same arrays, or the same status and line; returns the status"""
    status, line, m = run_abi(data, chunk, split)
    try:
        want = iref.csr_csc(iref.parse(data, max_line))
    except iref.Refused as e:
        assert (status, line) == (e.status, e.line), (status, line, str(e))
        return status
    assert status == 0, (status, line)
    got = indexes(m)
    assert same_index(got[0], want[0]) and same_index(got[1], want[1])
    return 0


def entry_lines(n, n_genes, start=0):
    """n entry lines with distinct (gene, cell) pairs and values that tell them apart"""
    return [b"%d %d %d\n" % ((start + i) % n_genes + 1, (start + i) // n_genes + 1, (start + i) * 7 % 1000) for i in range(n)]


def body_of(n_bytes, n_genes, tail=b""):
    """whole entry lines filling exactly n_bytes (the last one padded with blanks), then `tail`; returns (body, lines)"""
    lines, size = [], 0
    for ln in entry_lines(n_bytes // 6 + 1, n_genes):
        room = n_bytes - size - len(ln)
        if room < 16:                                           # no room for another line behind this one
            lines.append(ln[:-1] + b" " * room + b"\n")
            size = n_bytes
            break
        lines.append(ln)
        size += len(ln)
    assert size == n_bytes, (size, n_bytes)
    return b"".join(lines) + tail, len(lines)


def file_of(body, n_genes, n_cells, nnz):
    return HEAD + b"%d %d %d\n" % (n_genes, n_cells, nnz) + body


# ---- the golden directories ---------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("s", ["A", "B"])
def test_golden_equals_the_reference_at_every_chunking(gpu_lib, gold, s):
    data = mtx_bytes(gold, s)
    want = reference_indexes(gold, s)
    for chunk, split in ((0, 0), (64, 0), (0, 1), (64, 1), (4096, 1000)):
        status, line, m = run_abi(data, chunk, split)
        assert status == 0, (chunk, split, status, line)
        got = indexes(m)
        assert same_index(got[0], want[0]) and same_index(got[1], want[1]), (chunk, split)
        assert (m.n_genes, m.n_cells, m.max_value) == (200, 300, 2 ** 31 + 12345)


@pytest.mark.gpu
def test_read_mtx_takes_directories_files_and_streams(gpu_lib, gold, tmp_path):
    for s in ("A", "B"):
        where = write_dir(gold, s, tmp_path / s)
        want = reference_indexes(gold, s)
        name = "matrix.mtx" if s == "A" else "matrix.mtx.gz"
        f = files_of(gold, s)[name]
        for source in (where, os.path.join(where, name), gzip.open(io.BytesIO(f)) if s == "B" else io.BytesIO(f)):
            got = indexes(gpu_lib.read_mtx(source, chunk_bytes=8192))
            assert same_index(got[0], want[0]) and same_index(got[1], want[1]), (s, source)
    with pytest.raises(FileNotFoundError):
        gpu_lib.read_mtx(str(tmp_path))
    with pytest.raises(ValueError) as e:
        gpu_lib.read_mtx(io.BytesIO(file_of(b"1 1 1\n1 x 1\n", 5, 9, 2)))
    assert str(e.value).startswith("ERROR: line 4:")


@pytest.mark.gpu
def test_order_independence(gpu_lib, gold):
    data = mtx_bytes(gold, "A")
    pos = iref.parse_header(data)[4]
    lines = data[pos:].splitlines(True)
    np.random.default_rng(5).shuffle(lines)
    want = reference_indexes(gold, "A")
    status, _, m = run_abi(data[:pos] + b"".join(lines), 4096)
    got = indexes(m)
    assert status == 0 and same_index(got[0], want[0]) and same_index(got[1], want[1])


# ---- the edges of the geometry --------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_bodies_around_a_tile(gpu_lib, geo):
    T, ML = geo["tile_bytes"], geo["max_line"]
    for n_bytes in (T - 1, T, T + 1, 2 * T, 3 * T + 5):
        body, n = body_of(n_bytes, 50)
        assert len(body) == n_bytes
        assert agrees(file_of(body, 50, n // 50 + 1, n), ML) == 0
    # a line whose first byte is the last byte of a tile; one that ends exactly on a tile's end is the last of body_of(T)
    body, n = body_of(T - 1, 50)
    more = entry_lines(3, 50, start=n)
    assert (body + more[0])[T - 1:T] == more[0][:1] and body.endswith(b"\n")
    assert agrees(file_of(body + b"".join(more), 50, n // 50 + 2, n + 3), ML) == 0
    # ... without its final newline, and with \r\n
    assert agrees(file_of(body + b"".join(more)[:-1], 50, n // 50 + 2, n + 3), ML) == 0
    assert agrees(file_of((body + b"".join(more)).replace(b"\n", b"\r\n"), 50, n // 50 + 2, n + 3), ML) == 0


@pytest.mark.gpu
def test_the_longest_line(gpu_lib, geo):
    T, ML = geo["tile_bytes"], geo["max_line"]
    body, n = body_of(T - 1, 50)
    one = entry_lines(1, 50, start=n)[0][:-1]
    after = entry_lines(1, 50, start=n + 1)[0]
    # exactly max_line bytes, padded with blanks, from the last byte of a tile on: all of the look-ahead is read
    fits = one + b" " * (ML - len(one)) + b"\n"
    assert len(fits) == ML + 1
    assert agrees(file_of(body + fits + after, 50, n // 50 + 2, n + 2), ML) == 0
    assert agrees(file_of(fits + after, 50, n // 50 + 2, 2), ML) == 0
    # one byte more: refused, with its line
    over = one + b" " * (ML + 1 - len(one)) + b"\n"
    for data in (file_of(body + over + after, 50, n // 50 + 2, n + 2), file_of(over + after, 50, n // 50 + 2, 2),
                 file_of(body + b"%" + b"x" * ML + b"\n" + after, 50, n // 50 + 2, n + 1)):
        status, line, _ = run_abi(data)
        assert agrees(data, ML) == -1 and status == -1 and line == (2 + n + 1 if data.count(b"\n") > 10 else 3)
    # the same when the line never ends, fed in small pieces with a small chunk: the host sees it first
    data = file_of(b"1 1 1\n" + b"2" * (4 * ML), 50, 9, 2)
    assert agrees(data, ML, chunk=64, split=100) == -1 and run_abi(data, 64, 100)[1] == 4


def fill_points(body, chunk):
    """the offsets in the body at which a buffer of `chunk` bytes is full: the reader cuts the piece at the last \\n in front
    of such a point and carries the rest"""
    out, start = [], 0
    while start + chunk <= len(body):
        end = start + chunk
        out.append(end)
        start = body.rfind(b"\n", start, end) + 1
        assert start > 0
    return out


@pytest.mark.gpu
def test_chunk_boundaries_inside_fields(gpu_lib, geo):
    rng = np.random.default_rng(11)
    lines, where = [], []
    for i in range(400):
        f = [b"0" * int(rng.integers(0, 6)) + b"%d" % v for v in (i % 50 + 1, i // 50 + 1, i * 13 % 977)]
        gaps = [b" " * int(rng.integers(1, 4)) for _ in range(2)]
        lines.append(f[0] + gaps[0] + f[1] + gaps[1] + f[2] + b"\r\n")
        where.append("1" * len(f[0]) + " " * len(gaps[0]) + "2" * len(f[1]) + " " * len(gaps[1]) + "3" * len(f[2]) + "r" + "n")
    body, kinds = b"".join(lines), "".join(where)
    # a buffer fills in front of the byte at a fill point: inside a field when that byte and the one before belong to it
    cuts = {kinds[p - 1] + kinds[p] for p in fill_points(body, 64)}
    assert {"11", "22", "33", "rn"} <= cuts, cuts
    for split in (0, 1, 50):
        assert agrees(file_of(body, 50, 9, 400), geo["max_line"], chunk=64, split=split) == 0


# ---- the grammar ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_grammar_line_by_line(gpu_lib, geo):
    ML = geo["max_line"]
    assert ML == 1024                                           # LINES is written for it
    seen = set()
    for line, want in LINES:
        for tail in (b"\n", b""):
            data = file_of(b"2 2 2\n" + line + tail, 5, 9, 1 + isinstance(want, tuple))
            status, ln, m = run_abi(data, 4096)
            if isinstance(want, tuple):
                assert status == 0 and m.nnz == 2 and int(m.val[m.gene == want[0] - 1][-1]) == want[2], line
            elif want is None:
                assert status == 0 and m.nnz == 1, line
            else:
                assert (status, ln) == (-1, 4), line
            seen.add(agrees(data, ML, 4096))
    assert seen == {0, -1}
    # everything at once: tabs, runs of blanks, leading zeros, CRLF, blank and % lines in the body, a stored zero, the largest
    # value, no final newline
    good = b"\n".join([b"1 1 1", b"  3\t 2   7 \t", b"003 0003 0", b"3 4 7\r", b"", b" \t ", b"\r", b"% 1 2 x", b"  %", b"5 9 4294967295",
                       b"5 8 0000000000000000000000001", b"2\t2\t2"])
    n = 7
    assert agrees(file_of(good, 5, 9, n), ML, 4096) == 0 and agrees(file_of(good, 5, 9, n), ML, 64, 1) == 0
    status, _, m = run_abi(file_of(good, 5, 9, n), 64)
    assert status == 0 and 0 in m.val and 4294967295 in m.val and m.max_value == 4294967295


@pytest.mark.gpu
def test_headers(gpu_lib, geo):
    ML = geo["max_line"]
    for data in (b"", HEAD, HEAD + b"5 9\n", HEAD.replace(b"coordinate", b"array") + b"5 9 0\n", HEAD[1:] + b"5 9 0\n", HEAD + b"2147483648 9 0\n",
                 HEAD + b"5 2147483648 0\n", HEAD + b"%\n% two\n5 9 0", HEAD.upper().replace(b"%%MATRIXMARKET", b"%%MatrixMarket") + b"5 9 0\n",
                 HEAD.replace(b"integer", b"real") + b"%" + b"c" * 5000 + b"\n5 9 1\n3 3 3\n", HEAD + b"5 9 1\n1 1 3.0\n", HEAD + b"0 0 0\n"):
        for split in (0, 1):
            agrees(data, ML, 4096, split)
    from nabo_amd import _lib
    h = C.c_void_p()
    assert _lib.lib().nabo_mtx_create(0, 0, 1000, C.byref(h)) == 0                # a budget of 1000 bytes
    assert _lib.lib().nabo_mtx_feed(h, HEAD + b"5 9 1\n", len(HEAD) + 6) == _lib.E_NOMEM
    assert _lib.lib().nabo_mtx_feed(h, b"1 1 1\n", 6) == _lib.E_INVALID            # a failed reader takes nothing more
    _lib.lib().nabo_mtx_free(h)
    assert _lib.lib().nabo_mtx_create(99, 0, 0, C.byref(h)) == _lib.E_NODEVICE
    r = gpu_lib.MtxReader()
    assert _lib.lib().nabo_mtx_get_csr(r._h, None, None, None) == _lib.E_INVALID  # before finish
    r.feed(HEAD + b"5 9 0\n")
    m = r.finish()
    assert m.nnz == 0 and m.cell_ptr.tolist() == [0] * 10 and m.gene_ptr.tolist() == [0] * 6 and m.max_value == 0
    assert _lib.lib().nabo_mtx_feed(r._h, b"1 1 1\n", 6) == _lib.E_INVALID         # after finish
    ms, chunks = r.last_device_ms()
    assert chunks == 0 and set(ms) == {"upload", "parse", "sort", "transpose", "download"}
    r.close()


@pytest.mark.gpu
def test_the_lowest_bad_line_wins(gpu_lib, geo):
    T, ML = geo["tile_bytes"], geo["max_line"]
    lines = entry_lines(6000, 50)
    size = np.cumsum([len(x) for x in lines])
    assert size[-1] > 3 * T
    first, second = int(np.searchsorted(size, T + 100)), int(np.searchsorted(size, 2 * T + 100))     # lines in the second and third tile
    for bad in ((first, second), (second,), (first, 5999), (0, first)):
        mine = list(lines)
        for k, b in enumerate(bad):
            mine[b] = (b"1 1 -1\n", b"7 7 7 7\n")[k % 2]
        data = file_of(b"".join(mine), 50, 121, 6000)
        for chunk in (0, 20000):
            status, line, _ = run_abi(data, chunk)
            assert (status, line) == (-1, 2 + bad[0] + 1), (bad, chunk, line)
        assert agrees(data, ML) == -1


@pytest.mark.gpu
def test_entry_counts_and_duplicates(gpu_lib, geo):
    T, ML = geo["tile_bytes"], geo["max_line"]
    lines = entry_lines(4000, 50)
    body = b"".join(lines)
    assert len(body) > 2 * T

    def swap(k, new):
        return b"".join(lines[:k] + [new] + lines[k + 1:])
    for chunk in (0, 4096):
        # one too many: the first line in excess, in whatever chunk it stands; skipped lines do not count
        assert run_abi(file_of(body, 50, 81, 3999), chunk)[:2] == (-1, 2 + 4000)
        assert run_abi(file_of(swap(7, lines[7] + b"\n% c\n"), 50, 81, 3999), chunk)[:2] == (-1, 2 + 4002)
        assert run_abi(file_of(body, 50, 81, 10), chunk)[:2] == (-1, 2 + 11)
        # ... unless a bad line stands in front of it
        assert run_abi(file_of(swap(5, b"x\n"), 50, 81, 10), chunk)[:2] == (-1, 2 + 6)
        assert run_abi(file_of(swap(20, b"x\n"), 50, 81, 10), chunk)[:2] == (-1, 2 + 11)
        # one too few: at finish, the last line of the file
        assert run_abi(file_of(body, 50, 81, 4001), chunk)[:2] == (-1, 2 + 4000)
        for data in (file_of(body, 50, 81, 3999), file_of(body, 50, 81, 4001), file_of(body, 50, 81, 4000)):
            agrees(data, ML, chunk)
        # the same pair in the first and in the last line
        dup = file_of(body + lines[0].replace(b" 0\n", b" 5\n"), 50, 81, 4001)
        status, line, _ = run_abi(dup, chunk)
        from nabo_amd import _lib
        assert (status, line) == (-1, None) and "gene 1 of cell 1 " in _lib.lib().nabo_last_error().decode()
        assert agrees(dup, ML, chunk) == -1


# ---- size -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def million():
    """10^6 entries over 70 000 genes x 3 000 cells, shuffled: (text, the expected CSR and CSC)"""
    n_genes, n_cells, n = 70000, 3000, 1000000
    rng = np.random.default_rng(2024)
    flat = np.unique(rng.integers(0, n_genes * n_cells, size=n + n // 50))
    assert len(flat) >= n
    flat = rng.permutation(flat)[:n]
    gene, cell, val = flat % n_genes, flat // n_genes, rng.integers(0, 2 ** 32, size=n)
    text = iref.mtx_text(n_genes, n_cells, gene, cell, val)
    return text, iref.index_by(cell, gene, val, n_cells), iref.index_by(gene, cell, val, n_genes)


@pytest.mark.gpu
def test_a_million_entries_in_many_chunks(gpu_lib, geo, million):
    text, want_csr, want_csc = million
    r = gpu_lib.MtxReader(chunk_bytes=1 << 20)
    r.feed(text)
    m = r.finish()
    ms, chunks = r.last_device_ms()
    r.close()
    assert chunks > 12 and (1 << 20) // geo["tile_bytes"] == 64 and int(m.gene.max()) >= 2 ** 16
    got = indexes(m)
    assert same_index(got[0], want_csr) and same_index(got[1], want_csc)
    assert all(ms[k] > 0 for k in ms)
    # repeatability, and the default chunk (one piece, about a thousand tiles)
    again = indexes(gpu_lib.read_mtx(io.BytesIO(text), chunk_bytes=1 << 20))
    whole = indexes(gpu_lib.read_mtx(io.BytesIO(text)))
    for other in (again, whole):
        assert all(a.tobytes() == b.tobytes() for x, y in zip(got, other) for a, b in zip(x, y))


# ---- the transpose on its own ---------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_transpose_against_a_stable_argsort(gpu_lib, million):
    rng = np.random.default_rng(3)
    cases = [([0], [], [], 4), ([0, 0, 0], [], [], 1), ([0, 5], [0, 2, 3, 7, 9], rng.random(5), 10), ([0, 1, 1, 2, 3], [0, 0, 0], [1.5, 0.0, 2.5], 1),
             ([0, 0, 0, 2, 4, 4, 4], [1, 3, 0, 3], [1, 2, 3, 4], 5)]
    _, (cell_ptr, gene, val), _ = million
    cases.append((cell_ptr, gene, (val % 1000).astype(np.float32), 70000))
    for ptr, idx, v, n_cols in cases:
        got = gpu_lib.csr_to_csc(ptr, idx, v, n_cols)
        want = iref.transpose(ptr, idx, v, n_cols)
        assert got[0].dtype == np.int64 and got[1].dtype == np.int32 and got[2].dtype == np.float32
        assert all(np.array_equal(a, b) for a, b in zip(got, want)), (len(idx), n_cols)
    # the transpose of the transpose
    t = gpu_lib.csr_to_csc(*cases[-1])
    back = gpu_lib.csr_to_csc(t[0], t[1], t[2], 3000)
    assert np.array_equal(back[0], cell_ptr) and np.array_equal(back[1], gene) and np.array_equal(back[2], cases[-1][2])
    from nabo_amd import _lib
    L = _lib.lib()
    ptr, idx, v = np.array([0, 2, 3], np.int64), np.array([0, 2, 1], np.int32), np.ones(3, np.float32)
    out = [np.zeros(4, np.int64), np.zeros(3, np.int32), np.zeros(3, np.float32)]

    def call(ptr=ptr, idx=idx, v=v, n_rows=2, n_cols=3, device=0):
        return L.nabo_csr_transpose(device, n_rows, n_cols, ptr.ctypes.data, idx.ctypes.data, v.ctypes.data, *[x.ctypes.data for x in out])
    assert call() == 0 and out[0].tolist() == [0, 1, 2, 3] and out[1].tolist() == [0, 1, 0]
    assert call(ptr=np.array([0, 3, 2], np.int64)) == _lib.E_INVALID              # a non-monotone ptr
    assert call(idx=np.array([0, 3, 1], np.int32)) == _lib.E_INVALID              # an index out of range
    assert call(idx=np.array([2, 0, 1], np.int32)) == _lib.E_INVALID              # a row that is not strictly increasing
    assert call(idx=np.array([1, 1, 0], np.int32)) == _lib.E_INVALID
    assert call(n_cols=-1) == _lib.E_INVALID and call(device=99) == _lib.E_NODEVICE


# ---- the chain, the files, plain C ------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_chain_into_qc_and_gene_statistics(gpu_lib, gold, tmp_path):
    m = gpu_lib.read_mtx(write_dir(gold, "A", tmp_path / "A"))
    assert m.max_value >= 2 ** 24                               # (the one large value is rounded by float32, as documented)
    cls = (np.arange(m.n_genes) % 3 == 0).astype(np.uint8)
    cell_ptr, gene, val = m.csr()
    assert val.dtype == np.float32
    n_ent, sums = gpu_lib.cell_qc_csr(cell_ptr, gene, val, cls, 1)
    want = qref.cell_qc(cell_ptr, gene, val, cls, 1)
    assert np.array_equal(n_ent, want[0]) and np.array_equal(sums.view(np.int64), want[1].view(np.int64))
    assert np.array_equal(n_ent, np.diff(m.cell_ptr)) and sums[1, 0] > 2 ** 31
    sf = (1000.0 / np.maximum(sums[:, 0], 1.0)).astype(np.float32)
    st = gpu_lib.gene_stats_csc(*m.csc(sf))
    assert np.array_equal(st["ncells"], np.diff(m.gene_ptr)) and st["valid"].sum() > 100
    assert len(m.csr(sf)) == 4
    with pytest.raises(ValueError):
        m.csc(sf[:-1])


@pytest.mark.gpu
def test_file_level_mtx_to_h5(gpu_lib):
    py = _interpreter()
    if py is None:
        pytest.skip("no interpreter with h5py in this image")
    r = subprocess.run([py, os.path.join(HERE, "_ingest_case.py")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][len("RESULT "):])
    assert res["checked"] == 24 and res["differ"] == [], res


@pytest.mark.gpu
def test_plain_c_consumer(gpu_lib, gold, tmp_path):
    exe = build_ingest_check(tmp_path)
    data = mtx_bytes(gold, "B")
    r = subprocess.run([exe, "run", "1000"], input=data, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:]
    out = {ln.split()[0]: np.array(ln.split()[1:], dtype=np.int64) for ln in r.stdout.decode().splitlines()}
    (cell_ptr, gene, val), (gene_ptr, cell, gval) = reference_indexes(gold, "B")
    assert out["size"].tolist() == [200, 300, len(gene)]
    for name, want in (("cell_ptr", cell_ptr), ("gene", gene), ("val", val), ("gene_ptr", gene_ptr), ("cell", cell), ("gene_val", gval)):
        assert np.array_equal(out[name], want.astype(np.int64)), name
    r = subprocess.run([exe, "run", "7"], input=data.replace(b"\n", b"\n-\n", 9), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert r.returncode == 1 and r.stdout.startswith(b"error -1: line ")
