"""Local tournament seeds without a GPU: the layout rules the device kernels share with the host (nabo_amd/csrc/local_seeds.h,
compiled here with g++ through tests/local_seeds_host) against a plain restatement, and the planner's decision where a
launch takes them (nabo_query_plan, field "local_seed_buckets")."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from nabo_amd import _knn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COL = 128


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("lseed") / "liblseed_host.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-I" + os.path.join(REPO, "nabo_amd", "csrc"),
                           os.path.join(REPO, "tests", "local_seeds_host", "plan_shim.cpp"), "-o", so])
    L = C.CDLL(so)
    L.lseed_columns_host.restype = C.c_int64
    L.lseed_columns_host.argtypes = [C.c_int64, C.c_int]
    return L


def _tournament(L, lkeep, T):
    pt, gt = C.c_int(), C.c_int()
    L.lseed_tournament_host(lkeep, T, C.byref(pt), C.byref(gt))
    return pt.value, gt.value


def _layout(L, ref_cnt, row_cnt, cap, lkeep, tile0, rest):
    nb = len(ref_cnt)
    ref = np.ascontiguousarray(ref_cnt, dtype=np.uint32)
    lay = np.zeros(3 * (nb + 1), dtype=np.int64)
    if row_cnt is None:
        L.lseed_layout_host(nb, ref.ctypes.data_as(C.c_void_p), None, cap, lkeep, tile0, None, C.c_int64(0),
                            lay.ctypes.data_as(C.c_void_p), None)
        return lay.reshape(3, nb + 1), None
    row = np.ascontiguousarray(row_cnt, dtype=np.uint32)
    ncol = L.lseed_columns_host(int(row.sum()), nb)
    ranges = np.full((ncol, 4), -1, dtype=np.int32)
    r4 = (C.c_int * 4)(*rest)
    L.lseed_layout_host(nb, ref.ctypes.data_as(C.c_void_p), row.ctypes.data_as(C.c_void_p), cap, lkeep, tile0, r4, C.c_int64(ncol),
                        lay.ctypes.data_as(C.c_void_p), ranges.ctypes.data_as(C.c_void_p))
    return lay.reshape(3, nb + 1), ranges


@pytest.mark.parametrize("lkeep", [16, 23, 28, 32, 64])
def test_a_bucket_tournament_covers_its_whole_run_in_even_groups(shim, lkeep):
    q = (lkeep + 3) // 4
    for T in list(range(0, 6 * q + 3)) + [100, 255, 256, 511, 512, 1000, 1024]:
        pt, gt = _tournament(shim, lkeep, T)
        if T < 6 * q:                                   # fewer than 3 q groups of two tiles: no tournament (l2c_pre_plan's rule)
            assert pt == 0
            continue
        assert gt >= 2 and gt % 2 == 0 and gt <= 8
        assert pt % gt == 0 and T <= pt < T + gt         # whole groups; past the run's end only padding tiles
        assert pt // gt >= 3 * q                         # enough group minima for 4 lanes x q values


def test_reference_runs_are_fixed_slots_of_whole_tiles(shim):
    ref = [0, 1, 31, 32, 33, 5000, 16384, 20000]
    cap = 16384
    (base, padb, pade), _ = _layout(shim, ref, None, cap, 23, 0, None)
    for b, n in enumerate(ref):
        kept = min(n, cap)
        assert base[b] == b * cap and padb[b] == base[b] + kept
        assert pade[b] == base[b] + -(-kept // 32) * 32 and pade[b] <= base[b] + cap


def test_rows_are_laid_out_by_bucket_in_whole_columns_with_one_rest_class(shim):
    rng = np.random.default_rng(3)
    for trial in range(20):
        nb = int(rng.integers(1, 70))
        cap = int(rng.choice([1024, 4096, 16384]))
        lkeep = int(rng.choice([16, 23, 32, 64]))
        q = (lkeep + 3) // 4
        ref = rng.integers(0, 3 * cap, nb) * (rng.random(nb) < 0.8)
        ref[rng.integers(0, nb)] = 6 * q * 32 - 32      # one tile short of a tournament
        row = rng.integers(0, 1000, nb) * (rng.random(nb) < 0.8)
        tile0, rest = 31314, (0, 31250, 1035, 8)
        (base, padb, pade), ranges = _layout(shim, ref, row, cap, lkeep, tile0, rest)
        ncol = len(ranges)
        assert ncol == -(-int(row.sum()) // COL) + nb + 1
        T = -(-np.minimum(ref, cap) // 32)
        local = T >= 6 * q
        pos = 0
        want = np.zeros((ncol, 4), dtype=np.int64)
        for b in np.flatnonzero(local):                 # buckets with a tournament, in order, each in columns of its own
            assert base[b] == pos and padb[b] == pos + row[b]
            cols = -(-int(row[b]) // COL)
            pt, gt = _tournament(shim, lkeep, int(T[b]))
            t0 = tile0 + b * (cap // 32)
            assert t0 + T[b] <= tile0 + (b + 1) * (cap // 32)        # inside the bucket's slot
            want[pos // COL:pos // COL + cols] = (t0, t0 + T[b], pt, gt)
            pos += cols * COL
            assert pade[b] == pos
        assert base[nb] == pos                          # the rest class: every other bucket's rows back to back
        for b in np.flatnonzero(~local):
            assert base[b] == pos and padb[b] == pade[b] == 0
            pos += int(row[b])
        assert padb[nb] == pos
        cols = -(-(pos - int(base[nb])) // COL)
        want[base[nb] // COL:base[nb] // COL + cols] = rest
        assert pade[nb] == base[nb] + cols * COL and pade[nb] // COL <= ncol
        assert np.array_equal(ranges, want)             # (columns no class reaches: all zero, no tournament)


def test_every_bucket_too_small_leaves_one_rest_class(shim):
    (base, padb, pade), ranges = _layout(shim, [20] * 8, [5, 0, 300, 1, 0, 0, 77, 2], 16384, 23, 100, (0, 157, 32, 2))
    assert list(base) == [0, 5, 5, 305, 306, 306, 306, 383, 0] and padb[8] == 385 and pade[8] == 512
    assert (ranges[:4] == (0, 157, 32, 2)).all() and (ranges[4:] == 0).all()


def test_the_planner_takes_local_seeds_for_long_one_split_launches_only():
    P = lambda *a, **k: _knn.query_plan(*a, **k)["local_seed_buckets"]      # noqa: E731
    head = _knn.query_plan(1000000, 50, 1000000, 15)
    assert head["splits"] == 1 and head["local_seed_buckets"] == 64         # the headline's main launch
    assert P(1000000, 50, 1000000, 15, options={"local_seeds": 0}) == 0
    assert P(1000000, 50, 1000000, 15, options={"prepass": 0}) == 0         # no tournament at all
    assert P(1000000, 50, 1000000, 15, options={"local_anchors": 256}) == 256
    assert P(1000000, 50, 1000000, 15, options={"local_anchors": 1000}) == 256
    assert P(1000000, 50, 1000000, 15, l2_mode="f32") == 0                  # another first filter
    assert P(1000000, 100, 1000000, 50, metric=2) == 0                      # geometry C: measured slower, off by default
    assert P(1000000, 100, 1000000, 50, metric=2, options={"local_seeds": 2}) == 64
    assert P(1000000, 50, 1000000, 20) == 0                                 # geometry A: not measured, off by default
    assert P(100000, 50, 100000, 15) == 0                                   # cut into reference splits: per-split seeds stay
    assert P(200000, 50, 1000000, 15) == 0                                  # fewer than 2^18 references
    assert P(1000000, 50, 30000, 15, options={"splits": 1}) == 0            # fewer than 2^16 rows
    assert P(1000000, 50, 30000, 15, options={"splits": 1, "local_seeds": 2}) == 64
    assert P(5000, 50, 300, 15, options={"local_seeds": 2}) == 0            # one round of workgroups: reference splits
    assert P(5000, 50, 300, 15, options={"splits": 1, "local_seeds": 2, "local_anchors": 4}) == 4
    assert P(3, 50, 300, 2, options={"splits": 1, "local_seeds": 2, "local_anchors": 4}) == 0      # fewer references than anchors
