"""The table of bucket ends the two-level stream's mode control walks (nabo_amd/csrc/local_seeds.h: lseed_bucket_ends on the
layout of the full ordered copy), compiled for the host through tests/bucket_ends_host and held against a plain
restatement: bucket b ends ceil(count / 32) tiles behind its predecessor."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("bends") / "libbucket_ends_host.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-I" + os.path.join(REPO, "nabo_amd", "csrc"),
                           os.path.join(REPO, "tests", "bucket_ends_host", "ends_shim.cpp"), "-o", so])
    L = C.CDLL(so)
    L.lseed_bucket_ends_host.restype = C.c_int64
    L.lseed_bucket_ends_host.argtypes = [C.c_int, C.c_void_p, C.c_int64, C.c_void_p]
    return L


def _ends(L, cnt):
    """(ends, tiles of the ordered stream) for the unmasked references per bucket `cnt`, packed as the index packs them"""
    cnt = np.ascontiguousarray(cnt, dtype=np.uint32)
    end = np.full(len(cnt), -1, dtype=np.int32)
    ref_tiles = -(-int(cnt.sum(dtype=np.int64)) // 32)
    ot = L.lseed_bucket_ends_host(len(cnt), cnt.ctypes.data_as(C.c_void_p), ref_tiles, end.ctypes.data_as(C.c_void_p))
    return end, ot


def _check(L, cnt):
    end, ot = _ends(L, cnt)
    want, pos = [], 0
    for c in cnt:
        pos += -(-int(c) // 32)
        want.append(pos)
    assert end.tolist() == want
    assert (np.diff(end) >= 0).all() and (len(end) == 0 or end[0] >= 0)
    assert end[-1] <= ot and ot % 2 == 0


def test_the_ends_are_the_running_sum_of_whole_tiles(shim):
    rng = np.random.default_rng(17)
    for trial in range(200):
        nb = int(rng.integers(1, 257))
        kind = trial % 4
        if kind == 0:
            cnt = rng.integers(0, 40000, nb)
        elif kind == 1:
            cnt = rng.integers(0, 200, nb) * (rng.random(nb) < 0.6)              # many empty buckets
        elif kind == 2:
            cnt = rng.integers(0, 50, nb) * 32                                   # whole tiles, zeros among them
        else:
            cnt = rng.integers(0, 50, nb) * 32 + rng.choice([-1, 0, 1], nb)      # one cell either side of a whole tile
            cnt = np.maximum(cnt, 0)
        _check(shim, cnt)


def test_empty_buckets_repeat_an_end_and_short_ones_move_it_by_one(shim):
    end, ot = _ends(shim, [0, 0, 33, 0, 1, 32, 0])
    assert end.tolist() == [0, 0, 2, 2, 3, 4, 4] and ot == 10
    end, ot = _ends(shim, [0])
    assert end.tolist() == [0] and ot == 2
    # every bucket rounds up by less than a tile: the last end fits the stream even when each of C buckets wastes 31 cells
    end, ot = _ends(shim, [1] * 256)
    assert end[-1] == 256 and ot == (8 + 256 + 1) // 2 * 2
