"""The sub-order inside the buckets of the two-level stream's copies, without a GPU: the key rule of
nabo_amd/csrc/local_seeds.h (which references of a bucket are its sub-anchors, how they are ranked, which one a cell takes,
where the cell then lies; compiled here with g++ through tests/sub_order_host) against a numpy restatement.

The cells are small integers in float32: every product and sum of the nearest-sub-anchor rule is exact, so ties are real
ties and the restatement must agree to the position.  The ranking runs in float64 in the header's own order of operations."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from nabo_amd import _knn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ITERS = 8


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("lsub") / "liblsub_host.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-fPIC", "-shared",
                           "-I" + os.path.join(REPO, "nabo_amd", "csrc"),
                           os.path.join(REPO, "tests", "sub_order_host", "sub_shim.cpp"), "-o", so])
    return C.CDLL(so)


def _positions(L, nb, S, cells, bucket, by_index=False):
    cells = np.ascontiguousarray(cells, dtype=np.float32)
    bucket = np.ascontiguousarray(bucket, dtype=np.int32)
    pos = np.full(len(cells), -7, dtype=np.int64)
    L.lseed_sub_positions_host(nb, S, C.c_int64(len(cells)), cells.shape[1], cells.ctypes.data_as(C.c_void_p),
                               bucket.ctypes.data_as(C.c_void_p), int(by_index), pos.ctypes.data_as(C.c_void_p))
    return pos


def _ranks(pts, by_index):
    """the ranking of local_seeds.h: power iteration from the all-ones vector, sums in index order, ties by index"""
    S, dim = pts.shape
    if by_index:
        return list(range(S))
    p = [[float(x) for x in row] for row in pts]
    mean = []
    for d in range(dim):
        s = 0.0
        for j in range(S):
            s += p[j][d]
        mean.append(s / S)
    v = [1.0] * dim

    def proj(j):
        s = 0.0
        for d in range(dim):
            s += (p[j][d] - mean[d]) * v[d]
        return s

    for _ in range(ITERS):
        t = [proj(j) for j in range(S)]
        w = []
        for d in range(dim):
            s = 0.0
            for j in range(S):
                s += t[j] * (p[j][d] - mean[d])
            w.append(s)
        ss = 0.0
        for d in range(dim):
            ss += w[d] * w[d]
        if not (0.0 < ss < 1.7976931348623157e308):
            break
        inv = 1.0 / math.sqrt(ss)
        v = [x * inv for x in w]
    t = [proj(j) for j in range(S)]
    return [sum(1 for i in range(S) if t[i] < t[j] or (t[i] == t[j] and i < j)) for j in range(S)]


def _restate(nb, S, cells, bucket, by_index=False):
    cells = np.asarray(cells, dtype=np.float32)
    pos = np.full(len(cells), -1, dtype=np.int64)
    start = 0
    for b in range(nb):
        idx = np.flatnonzero(bucket == b)
        r = np.zeros(len(idx), dtype=np.int64)
        if S > 1 and len(idx) >= S:
            a = cells[idx[np.arange(S) * (len(idx) // S)]].astype(np.float64)
            rank = np.array(_ranks(a, by_index))
            score = (a * a).sum(1)[None, :] - 2.0 * cells[idx].astype(np.float64) @ a.T
            r = rank[np.argmin(score, axis=1)]              # (argmin: the first of equal scores, the lowest sub-anchor)
        pos[idx[np.argsort(r, kind="stable")]] = start + np.arange(len(idx))
        start += -(-len(idx) // 32) * 32
    return pos


def _data(seed, n, dim, nb, masked=0.1, small=()):
    """integer cells around nb centres; bucket -1 for a masked cell; the buckets in `small` keep only a few cells"""
    rng = np.random.default_rng(seed)
    bucket = rng.integers(0, nb, n).astype(np.int32)
    centres = rng.integers(-6, 7, (nb, dim))
    cells = (centres[bucket] + rng.integers(-3, 4, (n, dim))).astype(np.float32)
    bucket[rng.random(n) < masked] = -1
    for b, keep in small:
        idx = np.flatnonzero(bucket == b)
        bucket[idx[keep:]] = -1
    return cells, bucket


def test_the_option_is_clamped_and_zero_is_the_default(shim):
    default, top = shim.lseed_sub_default_host(), shim.lseed_sub_max_host()
    assert 1 <= default <= top == 64
    got = [shim.lseed_sub_count_host(v) for v in (0, 1, 2, 8, 64, 65, 10 ** 6, -1, -(10 ** 6))]
    assert got == [default, 1, 2, 8, 64, 64, 64, 1, 1]
    P = lambda **o: _knn.query_plan(20000, 50, 20000, 15, options=dict({"two_level": 2, "splits": 1}, **o))      # noqa: E731
    assert P(two_level_sub=8) == P(two_level_sub=1) == P(), "the sub-order moves cells inside buckets, never a launch plan"


@pytest.mark.parametrize("S", [2, 8, 32, 64])
@pytest.mark.parametrize("by_index", [False, True])
def test_positions_follow_the_rule(shim, S, by_index):
    nb = 7
    cells, bucket = _data(S, 3000, 6, nb, small=((2, S - 1), (4, S), (5, 0)))
    pos = _positions(shim, nb, S, cells, bucket, by_index)
    off = _positions(shim, nb, 1, cells, bucket)
    assert np.array_equal(off, _restate(nb, 1, cells, bucket)) and np.array_equal(off, _positions(shim, nb, 0, cells, bucket))
    assert np.array_equal(pos, _restate(nb, S, cells, bucket, by_index))
    assert np.array_equal(pos, _positions(shim, nb, S, cells, bucket, by_index)), "the same call, the same positions"
    assert ((pos == -1) == (bucket == -1)).all()
    moved = 0
    for b in range(nb):
        idx = np.flatnonzero(bucket == b)
        assert sorted(pos[idx]) == sorted(off[idx]), "a permutation inside the bucket: its range and its end stay"
        if len(idx) < S:
            assert np.array_equal(pos[idx], off[idx]), "a bucket with fewer than S cells keeps its order"
        moved += int((pos[idx] != off[idx]).sum())
    assert moved > 0
    assert len(np.flatnonzero(bucket == 2)) == S - 1 and len(np.flatnonzero(bucket == 4)) == S


def test_equal_cells_keep_caller_order_and_ties_go_to_the_lowest_sub_anchor(shim):
    S, nb = 4, 1
    # sub-anchors: cells 0, 3, 6, 9 of 12 -- 0 and 3 are the same point, every copy of it must take sub-anchor 0
    pts = np.array([[0, 0], [5, 5], [1, 0], [0, 0], [9, 9], [0, 1], [4, 0], [0, 0], [3, 3], [0, 4], [0, 0], [4, 4]], dtype=np.float32)
    bucket = np.zeros(len(pts), dtype=np.int32)
    pos = _positions(shim, nb, S, pts, bucket)
    assert np.array_equal(pos, _restate(nb, S, pts, bucket))
    same = [0, 2, 3, 5, 7, 10]       # the copies of (0, 0), and (1, 0) and (0, 1) next to it: sub-anchor 1 gets nobody
    assert list(np.diff(pos[same])) == [1] * 5, "equal cells: one class, caller order, back to back"
    # (3, 3) is as far from (4, 0) as from (0, 4): the lower sub-anchor takes it, so it lies in the class of (4, 0)
    by_index = _positions(shim, nb, S, pts, bucket, True)
    assert np.array_equal(by_index, _restate(nb, S, pts, bucket, True))
    assert by_index[6] < by_index[8] < by_index[9] and by_index[8] == by_index[6] + 1


def test_the_ranking_orders_points_on_a_line_and_breaks_ties_by_index(shim):
    line = np.array([[3, 6, 0], [1, 2, 0], [4, 8, 0], [1, 2, 0], [0, 0, 0], [2, 4, 0]], dtype=np.float32)
    rank = np.zeros(len(line), dtype=np.uint8)
    shim.lseed_sub_ranks_host(len(line), 3, line.ctypes.data_as(C.c_void_p), 0, rank.ctypes.data_as(C.c_void_p))
    assert list(rank) == _ranks(line, False)
    assert list(rank) in ([4, 1, 5, 2, 0, 3], [1, 3, 0, 4, 5, 2]), "along the line, either way; the two equal points by index"
    same = np.ones((5, 4), dtype=np.float32)
    shim.lseed_sub_ranks_host(5, 4, same.ctypes.data_as(C.c_void_p), 0, rank.ctypes.data_as(C.c_void_p))
    assert list(rank[:5]) == [0, 1, 2, 3, 4], "no direction at all: by index"
