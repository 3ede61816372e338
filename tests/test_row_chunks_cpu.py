"""How the row steps (QC, projection, fit) cut their rows into chunks and gather a chunk, without a GPU:
nabo_amd/csrc/row_chunks.h, compiled here with g++ through tests/row_chunks_host.  The rule: a row costs
fixed + 8 bytes per entry; it joins the current chunk unless that takes the chunk past the room or the chunk holds `cap`
rows already; a row that alone exceeds the room is named with its bytes."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AMPLE = 1 << 40


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("row_chunks") / "librow_chunks_host.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-fPIC", "-shared",
                           "-I" + os.path.join(REPO, "nabo_amd", "csrc"), os.path.join(REPO, "tests", "row_chunks_host", "shim.cpp"),
                           "-o", so])
    L = C.CDLL(so)
    vp, i64 = C.c_void_p, C.c_int64
    L.rc_plan.restype = i64
    L.rc_plan.argtypes = [i64, vp, vp, i64, i64, i64, vp, vp]
    L.rc_gather.restype = i64
    L.rc_gather.argtypes = [i64, i64] + [vp] * 10
    return L


def ptr_of(entries):
    p = np.zeros(len(entries) + 1, dtype=np.int64)
    np.cumsum(entries, out=p[1:])
    return p


def plan(L, cell_ptr, fixed, room, cap=AMPLE, rows=None):
    """(chunk_start, max_rows, max_nnz), or ("oversize", row, bytes)"""
    cell_ptr = np.ascontiguousarray(cell_ptr, dtype=np.int64)
    rows = None if rows is None else np.ascontiguousarray(rows, dtype=np.int64)
    n_rows = cell_ptr.shape[0] - 1 if rows is None else rows.shape[0]
    start, out = np.full(n_rows + 2, -7, dtype=np.int64), np.zeros(4, dtype=np.int64)
    n = L.rc_plan(n_rows, None if rows is None else rows.ctypes.data, cell_ptr.ctypes.data, fixed, room, cap, start.ctypes.data, out.ctypes.data)
    if out[2] >= 0:
        return "oversize", int(out[2]), int(out[3])
    return start[:n].tolist(), int(out[0]), int(out[1])


def plan_ref(entries, fixed, room, cap):
    """the loop the three steps each had, on the entries per row"""
    start, used, nnz, max_rows, max_nnz = [0], 0, 0, 0, 0
    for r, ne in enumerate(entries):
        b = fixed + 8 * ne
        if b > room:
            return "oversize", r, b
        if r > start[-1] and (used + b > room or r - start[-1] >= cap):
            start.append(r)
            used = nnz = 0
        used, nnz = used + b, nnz + ne
        max_rows, max_nnz = max(max_rows, r + 1 - start[-1]), max(max_nnz, nnz)
    return start + [len(entries)], max_rows, max_nnz


def test_no_rows(shim):
    assert plan(shim, [0], 16, 100) == ([0, 0], 0, 0)
    assert plan(shim, [0, 3], 16, 100, rows=[]) == ([0, 0], 0, 0)


def test_one_row_exactly_at_the_room_and_one_byte_less(shim):
    assert plan(shim, [0, 5], 16, 56) == ([0, 1], 1, 5)
    assert plan(shim, [0, 5], 16, 55) == ("oversize", 0, 56)


@pytest.mark.parametrize("room,want", [(48, [0, 2, 3]), (47, [0, 1, 2, 3]), (72, [0, 3])])
def test_three_rows_of_24_bytes(shim, room, want):
    got = plan(shim, [0, 1, 2, 3], 16, room)
    assert got == (want, max(np.diff(want)), max(np.diff(want)))


def test_the_cap_on_rows(shim):
    assert plan(shim, ptr_of([3, 0, 1, 2, 5]), 16, AMPLE, cap=2) == ([0, 2, 4, 5], 2, 5)


def test_a_row_list_that_repeats_runs_backwards_and_names_empty_cells(shim):
    cell_ptr = ptr_of([4, 0, 1, 0, 6])                      # cells 1 and 3 are empty
    rows = [4, 4, 3, 2, 1, 0, 4]                            # entries per row: 6 6 0 1 0 4 6
    # fixed 8: the rows cost 56 56 8 16 8 40 56; room 112 -> [4 4] [3 2 1 0] [4]
    assert plan(shim, cell_ptr, 8, 112, rows=rows) == ([0, 2, 6, 7], 4, 12)
    # no slice of the matrix that 112 bytes hold has more than 6 entries: max_nnz above counts the gathered chunk [4 4]
    assert plan(shim, cell_ptr, 8, 112) == ([0, 4, 5], 4, 6)
    # the oversize answer names the position in rows, not the cell: row 5 is cell 0, the first of 40 bytes
    assert plan(shim, cell_ptr, 8, 39, rows=[3, 2, 1, 2, 1, 0, 4]) == ("oversize", 5, 40)


def test_random_cases_against_the_loop(shim):
    rng = np.random.default_rng(20261019)
    split3 = 0
    for case in range(200):
        n_cells = int(rng.integers(1, 41))
        entries = rng.integers(0, 13, size=n_cells)
        cell_ptr = ptr_of(entries)
        rows = rng.integers(0, n_cells, size=int(rng.integers(0, 41))) if case % 2 else None
        per_row = entries if rows is None else entries[rows]
        fixed = int(rng.choice([0, 12, 16, 24]))
        cost = fixed + 8 * per_row
        big = int(cost.max()) if cost.size else 0
        room = int(rng.integers(big, max(big, int(cost.sum()) // int(rng.integers(1, 8))) + 1)) - (case % 10 == 9)    # every tenth: oversize
        cap = int(rng.integers(1, 6)) if case % 5 == 4 else AMPLE
        want = plan_ref(per_row.tolist(), fixed, room, cap)
        assert plan(shim, cell_ptr, fixed, room, cap, rows) == want, (case, entries, rows, fixed, room, cap)
        split3 += want[0] != "oversize" and len(want[0]) >= 4
    assert split3 >= 50, "only %d of 200 cases split into three or more chunks" % split3


def matrix():
    """seven cells, the third and the last empty"""
    cell_ptr = ptr_of([3, 1, 0, 4, 2, 5, 0])
    n = int(cell_ptr[-1])
    return cell_ptr, np.arange(100, 100 + n, dtype=np.int32), np.arange(n, dtype=np.float32) * 0.5, np.arange(1, 8, dtype=np.float32)


def gather(L, r0, nr, m, rows=None, with_sf=True):
    cell_ptr, gene, val, sf = m
    rows = None if rows is None else np.ascontiguousarray(rows, dtype=np.int64)
    n = int(cell_ptr[-1]) * 3
    h_ptr, h_sf = np.full(nr + 1, -7, dtype=np.int64), np.full(nr, -7, dtype=np.float32)
    h_gene, h_val, src = np.full(n, -7, dtype=np.int32), np.full(n, -7, dtype=np.float32), (C.c_void_p * 2)()
    nnz = L.rc_gather(r0, nr, cell_ptr.ctypes.data, gene.ctypes.data, val.ctypes.data, sf.ctypes.data if with_sf else None,
                      None if rows is None else rows.ctypes.data, h_ptr.ctypes.data, h_sf.ctypes.data if with_sf else None,
                      h_gene.ctypes.data, h_val.ctypes.data, src)
    return nnz, h_ptr, h_sf, h_gene, h_val, (src[0], src[1])


@pytest.mark.parametrize("r0,nr", [(0, 7), (0, 3), (2, 4), (3, 1), (6, 1)])
def test_gather_without_rows_is_a_slice_of_the_callers_arrays(shim, r0, nr):
    m = matrix()
    cell_ptr, gene, val, sf = m
    nnz, h_ptr, h_sf, h_gene, h_val, src = gather(shim, r0, nr, m)
    e0 = int(cell_ptr[r0])
    assert nnz == cell_ptr[r0 + nr] - e0
    assert h_ptr.tolist() == (cell_ptr[r0:r0 + nr + 1] - e0).tolist()
    assert h_sf.tolist() == sf[r0:r0 + nr].tolist()
    assert src == (gene.ctypes.data + 4 * e0, val.ctypes.data + 4 * e0)
    assert (h_gene == -7).all() and (h_val == -7).all()                 # nothing is copied
    assert gather(shim, r0, nr, m, with_sf=False)[1].tolist() == h_ptr.tolist()


@pytest.mark.parametrize("r0,nr", [(0, 9), (0, 3), (3, 4), (2, 1), (8, 1)])
def test_gather_with_rows_concatenates_in_row_order(shim, r0, nr):
    m = matrix()
    cell_ptr, gene, val, sf = m
    rows = np.array([5, 5, 2, 0, 6, 3, 1, 0, 4])                        # repeats, backwards, the empty cells 2 and 6
    nnz, h_ptr, h_sf, h_gene, h_val, src = gather(shim, r0, nr, m, rows)
    mine = rows[r0:r0 + nr]
    pieces = [np.arange(cell_ptr[c], cell_ptr[c + 1]) for c in mine]
    at = np.concatenate(pieces)
    assert nnz == at.shape[0]
    assert h_ptr.tolist() == [0] + np.cumsum([p.shape[0] for p in pieces]).tolist()
    assert h_gene[:nnz].tolist() == gene[at].tolist() and h_val[:nnz].tolist() == val[at].tolist()
    assert (h_gene[nnz:] == -7).all() and (h_val[nnz:] == -7).all()
    assert h_sf.tolist() == sf[mine].tolist()
    assert src == (h_gene.ctypes.data, h_val.ctypes.data)
    assert gather(shim, r0, nr, m, rows, with_sf=False)[3].tolist() == h_gene.tolist()
