"""The simple graph the layout, the clustering and the potential start from, without a GPU: nabo_amd/csrc/simple_graph.h,
compiled here with g++ through tests/simple_graph_host, against the restatements the steps' own tests use
(_layout_ref.Graph for weighted input, _potential_ref.Graph for weight-less input)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _layout_ref as lr
import _potential_ref as pr
from nabo_amd import _community, _potential

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("simple_graph") / "libsimple_graph_host.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-fPIC", "-shared",
                           "-I" + os.path.join(REPO, "nabo_amd", "csrc"), os.path.join(REPO, "tests", "simple_graph_host", "shim.cpp"),
                           "-o", so])
    L = C.CDLL(so)
    vp, i64 = C.c_void_p, C.c_int64
    L.sg_pairs.restype = vp
    L.sg_pairs.argtypes = [i64, vp, vp, C.c_int]
    L.sg_rows.restype = None
    L.sg_rows.argtypes = [vp, i64, vp]
    L.sg_sizes.restype = None
    L.sg_sizes.argtypes = [vp, C.POINTER(i64)]
    L.sg_get.restype = None
    L.sg_get.argtypes = [vp] * 7
    L.sg_free.restype = None
    L.sg_free.argtypes = [vp]
    L.sg_long_rows.restype = i64
    L.sg_long_rows.argtypes = [i64, vp, i64, vp]
    return L


def csr(n, arcs):
    """arcs: (row, neighbour, weight) in CSR order"""
    rows = np.array([a[0] for a in arcs], dtype=np.int64)
    assert (np.diff(rows) >= 0).all()
    ptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=n), out=ptr[1:])
    return ptr, np.array([a[1] for a in arcs], dtype=np.int64), np.array([a[2] for a in arcs], dtype=np.float64)


def dirty6():
    """Pair (1, 4) from both ends with three weights: the lower-numbered row lists it twice, and the last occurrence (in a
    CSR the highest position always lies in the higher-numbered row) carries the weight that wins, 0.7.  Pair (0, 2) twice
    within row 0, a self-loop on 3 listed twice and 3's only arc, node 5 without any arc."""
    return csr(6, [(0, 2, 0.1), (0, 1, 0.6), (0, 2, 0.2), (1, 4, 0.5), (1, 4, 0.9), (2, 4, 0.8), (3, 3, 0.3), (3, 3, 0.4), (4, 1, 0.7)])


def build(L, ptr, nbr, weighted, keep_of=None):
    """the builder's arrays; keep_of(pairs, last) -> bool per pair, the drop predicate between the two steps"""
    n = len(ptr) - 1
    ptr, nbr = np.ascontiguousarray(ptr, dtype=np.int64), np.ascontiguousarray(nbr, dtype=np.int64)
    h = L.sg_pairs(n, ptr.ctypes.data, nbr.ctypes.data, int(weighted))
    try:
        def get():
            sz = (C.c_int64 * 6)()
            L.sg_sizes(h, sz)
            a = [np.zeros(sz[0], dtype=np.uint64), np.zeros(sz[1], dtype=np.int64), np.zeros(sz[2], dtype=np.int64),
                 np.zeros(sz[3], dtype=np.int32), np.zeros(sz[4], dtype=np.int64), np.zeros(sz[5], dtype=np.int64)]
            L.sg_get(h, *[x.ctypes.data for x in a])
            return dict(zip(("pairs", "last", "rptr", "rnbr", "slot_pair", "visited"), a))
        keep = None
        if keep_of is not None:
            first = get()
            keep = np.ascontiguousarray(keep_of(first["pairs"], first["last"]), dtype=np.uint8)
            assert keep.shape == first["pairs"].shape
        L.sg_rows(h, n, None if keep is None else keep.ctypes.data)
        out = get()
        out["keep"] = np.ones(len(out["pairs"]), dtype=bool) if keep is None else keep.astype(bool)
        assert out["visited"].tolist() == np.flatnonzero(out["keep"]).tolist()      # every kept pair once, in (a, b) order
        return out
    finally:
        L.sg_free(h)


def check_weighted(L, ptr, nbr, w, drop_zero=False):
    """against _layout_ref.Graph; drop_zero: the pairs whose (last) weight is 0 go before the rows are formed"""
    n, E = len(ptr) - 1, len(nbr)
    g = build(L, ptr, nbr, True, (lambda pairs, last: w[last] != 0) if drop_zero else None)
    G = lr.Graph(ptr, nbr, w)
    on = G.w != 0 if drop_zero else np.ones(len(G.w), dtype=bool)
    src, dst, gw = G.src[on], G.dst[on], G.w[on]
    want_ptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(src, minlength=n), out=want_ptr[1:])
    assert g["rptr"].tolist() == want_ptr.tolist()
    assert g["rnbr"].tolist() == dst.tolist()
    assert w[g["last"][g["slot_pair"]]].tolist() == gw.tolist()
    # the pairs: strictly ascending, every (a <= b) of the input once, self-loops included; last = the highest position
    lo, hi = (g["pairs"] >> np.uint64(32)).astype(np.int64), (g["pairs"] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    assert (lo <= hi).all() and (g["pairs"][1:] > g["pairs"][:-1]).all()
    row = np.repeat(np.arange(n), np.diff(ptr))
    key = np.minimum(row, nbr) * n + np.maximum(row, nbr)
    assert (lo * n + hi).tolist() == np.unique(key).tolist()
    top = np.full(n * n, -1, dtype=np.int64)
    np.maximum.at(top, key, np.arange(E))
    assert g["last"].tolist() == top[lo * n + hi].tolist()
    # the mass the layout takes off the pairs: 1 + the pairs at a node, a self-loop once
    deg = np.bincount(lo, minlength=n) + np.bincount(hi[hi != lo], minlength=n)
    assert (1.0 + deg).tolist() == G.mass.tolist()
    # slot -> pair: the pair of (row, neighbour), kept, and each kept pair off the diagonal at exactly its two slots
    srow = np.repeat(np.arange(n), np.diff(g["rptr"]))
    sp = g["slot_pair"]
    assert len(sp) == len(g["rnbr"])
    assert lo[sp].tolist() == np.minimum(srow, g["rnbr"]).tolist() and hi[sp].tolist() == np.maximum(srow, g["rnbr"]).tolist()
    assert g["keep"][sp].all()
    assert np.bincount(sp, minlength=len(lo)).tolist() == (2 * (g["keep"] & (lo != hi))).tolist()
    return g


def check_plain(L, ptr, nbr):
    """weight-less input against _potential_ref.Graph: the same rows, no occurrence index and no slot map"""
    g = build(L, ptr, nbr, False)
    G = pr.Graph(ptr, nbr)
    assert g["rptr"].tolist() == G.ptr.tolist() and g["rnbr"].tolist() == G.dst.tolist()
    assert len(g["last"]) == 0 and len(g["slot_pair"]) == 0
    lo, hi = (g["pairs"] >> np.uint64(32)).astype(np.int64), (g["pairs"] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    assert (lo <= hi).all() and (g["pairs"][1:] > g["pairs"][:-1]).all()
    assert np.bincount(lo[lo == hi], minlength=G.n).tolist() == G.loop.tolist()
    return g


@pytest.mark.parametrize("name", ["one_node", "one_loop", "four_nodes_no_arc", "dirty6", "random200"])
def test_builder_equals_the_restatements(shim, name):
    if name == "one_node":
        ptr, nbr, w = csr(1, [])
    elif name == "one_loop":
        ptr, nbr, w = csr(1, [(0, 0, 2.5)])
    elif name == "four_nodes_no_arc":
        ptr, nbr, w = csr(4, [])
    elif name == "dirty6":
        ptr, nbr, w = dirty6()
    else:
        rng = np.random.default_rng(20)
        rows = np.sort(rng.integers(0, 200, 3000))
        # neighbours near the row, so that pairs repeat from both ends and loops occur
        cols = np.clip(rows + rng.integers(-6, 7, 3000), 0, 199)
        ptr, nbr, w = csr(200, list(zip(rows.tolist(), cols.tolist(), rng.integers(1, 9, 3000) / 8.0)))
        key = np.minimum(rows, cols) * 200 + np.maximum(rows, cols)
        assert len(np.unique(key)) < 2500 and (rows == cols).sum() > 50
    g = check_weighted(shim, ptr, nbr, w)
    check_plain(shim, ptr, nbr)
    if name == "dirty6":
        assert g["rptr"].tolist() == [0, 2, 4, 6, 6, 8, 8]
        assert g["rnbr"].tolist() == [1, 2, 0, 4, 0, 4, 1, 2]
        assert w[g["last"][g["slot_pair"]]].tolist() == [0.6, 0.2, 0.6, 0.7, 0.2, 0.8, 0.7, 0.8]
        assert len(g["pairs"]) == 5 and w[g["last"]].tolist() == [0.6, 0.2, 0.7, 0.8, 0.4]


@pytest.mark.parametrize("name", ["middle_of_a_row", "a_row_becomes_empty", "all_pairs", "random200"])
def test_dropped_pairs_leave_before_the_rows_are_formed(shim, name):
    if name == "middle_of_a_row":          # row 2 is 0, 1, 3, 4: the pair (1, 2) and (2, 3) go from its middle
        ptr, nbr, w = csr(5, [(0, 2, 1.0), (1, 2, 0.0), (2, 3, 5.0), (2, 4, 1.0), (3, 2, 0.0), (3, 4, 2.0)])
    elif name == "a_row_becomes_empty":    # node 3 keeps no arc, nor does its loop weigh anything
        ptr, nbr, w = csr(4, [(0, 1, 1.0), (0, 3, 0.0), (1, 2, 1.0), (3, 2, 0.0), (3, 3, 0.0)])
    elif name == "all_pairs":
        ptr, nbr, w = csr(3, [(0, 1, 0.0), (1, 2, 0.0), (2, 0, 0.0), (2, 2, 0.0)])
    else:
        rng = np.random.default_rng(21)
        rows = np.sort(rng.integers(0, 200, 3000))
        cols = np.clip(rows + rng.integers(-6, 7, 3000), 0, 199)
        ptr, nbr, w = csr(200, list(zip(rows.tolist(), cols.tolist(), rng.integers(0, 3, 3000) / 2.0)))
    g = check_weighted(shim, ptr, nbr, w, drop_zero=True)
    assert not g["keep"].all()
    if name == "middle_of_a_row":
        assert g["rptr"].tolist() == [0, 1, 1, 3, 4, 6] and g["rnbr"].tolist() == [2, 0, 4, 4, 2, 3]
    if name == "a_row_becomes_empty":
        assert g["rptr"].tolist() == [0, 1, 3, 4, 4]
    if name == "all_pairs":
        assert g["rptr"].tolist() == [0, 0, 0, 0] and len(g["rnbr"]) == 0 and len(g["pairs"]) == 4


@pytest.mark.parametrize("step", ["community", "potential"])
def test_long_rows_start_one_past_the_threshold(shim, step):
    t = (_community.geometry() if step == "community" else _potential.geometry())[1]
    assert t >= 1
    # hub 0 has t + 1 partners, hub 1 exactly t
    arcs = [(0, j, 1.0) for j in range(2, t + 3)] + [(1, j, 1.0) for j in range(2, t + 2)]
    ptr, nbr, _ = csr(t + 3, arcs)
    g = check_plain(shim, ptr, nbr)
    deg = np.diff(g["rptr"])
    assert deg[0] == t + 1 and deg[1] == t
    out = np.full(t + 3, -1, dtype=np.int32)
    cnt = shim.sg_long_rows(t + 3, g["rptr"].ctypes.data, t, out.ctypes.data)
    assert out[:cnt].tolist() == [0] and pr.Graph(ptr, nbr).c.tolist() == deg.tolist()
