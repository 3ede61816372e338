"""Whether an index's data takes the two-level stream, without a GPU: the remembered verdict and its rules
(nabo_amd/csrc/two_level_verdict.h, compiled here with g++ through tests/two_level_verdict_host) against a plain restatement
with the numbers written out -- 30 % one-step tiles in a probe, one-step x 3 against two-step in a launch of at least 1024
rows, a probe from 512 ordered workgroups and 4096 ordered tiles on, forgotten at the 16th repack."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOT_KNOWN, STREAMS, CALLER_ORDER = 0, 1, 2


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("tlverdict") / "libtlverdict_host.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fPIC", "-shared", "-I" + os.path.join(REPO, "nabo_amd", "csrc"),
                           os.path.join(REPO, "tests", "two_level_verdict_host", "verdict_shim.cpp"), "-o", so])
    L = C.CDLL(so)
    u64, i64, ip = C.c_uint64, C.c_int64, C.POINTER(C.c_int)
    L.tl_probe_due_host.argtypes = [ip, C.c_int, i64, i64]
    L.tl_probe_verdict_host.argtypes = [u64, u64]
    L.tl_launch_says_no_host.argtypes = [i64, C.c_int, u64, u64]
    for f in (L.tl_fresh_host, L.tl_known_host, L.tl_streams_host, L.tl_repack_host):
        f.argtypes = [ip]
    L.tl_give_host.argtypes = [ip, C.c_int]
    return L


def _v(state=NOT_KNOWN, age=0):
    return (C.c_int * 2)(state, age)


# ---- the restatement ----
def probe_due(state, two_level, wgs, tiles):
    return state == NOT_KNOWN and two_level == 1 and wgs >= 512 and tiles >= 4096


def probe_verdict(one_step, two_step):
    return CALLER_ORDER if 10 * one_step < 3 * (one_step + two_step) else STREAMS


def launch_says_no(m, coarse_adapt, one_step, two_step):
    return coarse_adapt != 0 and m >= 1024 and one_step * 3 < two_step


def repack(state, age):
    age += 1
    return (NOT_KNOWN, 0) if age >= 16 else (state, age)


def test_the_constants_and_states_are_the_documented_ones(shim):
    c = np.zeros(9, dtype=np.int64)
    shim.tl_constants_host(c.ctypes.data_as(C.c_void_p))
    assert list(c) == [16, 128, 1024, 512, 4096, 3, 10, 3, 1024]
    s = (C.c_int * 3)()
    shim.tl_states_host(s)
    assert list(s) == [NOT_KNOWN, STREAMS, CALLER_ORDER]
    v = _v(7, 7)
    shim.tl_fresh_host(v)
    assert list(v) == [NOT_KNOWN, 0]
    # not known: the stream is taken (a long query probes); only "no" sends the queries to the caller-order stream
    assert [shim.tl_known_host(_v(s)) for s in (0, 1, 2)] == [0, 1, 1]
    assert [shim.tl_streams_host(_v(s)) for s in (0, 1, 2)] == [1, 1, 0]


def test_a_probe_says_no_below_thirty_percent_one_step_tiles(shim):
    assert shim.tl_probe_verdict_host(3, 7) == STREAMS               # the boundary 3 (a + c) == 10 a exactly: 30 % is enough
    assert shim.tl_probe_verdict_host(3, 8) == CALLER_ORDER
    assert shim.tl_probe_verdict_host(4, 7) == STREAMS
    assert shim.tl_probe_verdict_host(300000, 700000) == STREAMS and shim.tl_probe_verdict_host(299999, 700001) == CALLER_ORDER
    assert shim.tl_probe_verdict_host(0, 0) == STREAMS and shim.tl_probe_verdict_host(0, 1) == CALLER_ORDER
    rng = np.random.default_rng(1)
    for a, c in itertools.chain(rng.integers(0, 200, (300, 2)), rng.integers(0, 1 << 40, (300, 2))):
        a, c = int(a), int(c)
        assert shim.tl_probe_verdict_host(a, c) == probe_verdict(a, c), (a, c)
        for a2 in (3 * c // 7 - 1, 3 * c // 7, 3 * c // 7 + 1):     # either side of 3 (a + c) == 10 a
            if a2 >= 0:
                assert shim.tl_probe_verdict_host(a2, c) == probe_verdict(a2, c), (a2, c)


def test_a_launch_says_no_when_one_step_tiles_times_three_stay_below_two_step(shim):
    assert shim.tl_launch_says_no_host(1100, 1, 10, 31) == 1
    assert shim.tl_launch_says_no_host(1100, 1, 10, 30) == 0         # 3 x one-step == two-step: stays
    assert shim.tl_launch_says_no_host(1100, 1, 10, 29) == 0
    assert shim.tl_launch_says_no_host(1024, 1, 10, 31) == 1 and shim.tl_launch_says_no_host(1023, 1, 10, 31) == 0      # off below m = 1024
    assert shim.tl_launch_says_no_host(1 << 20, 0, 10, 31) == 0      # off with coarse_adapt = 0
    assert shim.tl_launch_says_no_host(1 << 20, 1, 0, 0) == 0 and shim.tl_launch_says_no_host(1 << 20, 1, 0, 1) == 1
    rng = np.random.default_rng(2)
    for m, adapt, a in zip(rng.choice([1, 1000, 1023, 1024, 1025, 200000], 300), rng.integers(0, 3, 300), rng.integers(0, 1 << 40, 300)):
        for c in (3 * int(a) - 1, 3 * int(a), 3 * int(a) + 1, int(rng.integers(0, 1 << 42))):
            if c >= 0:
                assert shim.tl_launch_says_no_host(int(m), int(adapt), int(a), c) == launch_says_no(int(m), int(adapt), int(a), c), (m, adapt, a, c)


def test_a_probe_is_due_only_for_an_unknown_verdict_under_the_default_option_on_long_launches(shim):
    assert shim.tl_probe_due_host(_v(NOT_KNOWN), 1, 512, 4096) == 1
    assert shim.tl_probe_due_host(_v(STREAMS), 1, 512, 4096) == 0 and shim.tl_probe_due_host(_v(CALLER_ORDER), 1, 512, 4096) == 0
    assert shim.tl_probe_due_host(_v(NOT_KNOWN, 9), 1, 512, 4096) == 1              # (the age plays no part)
    assert shim.tl_probe_due_host(_v(NOT_KNOWN), 0, 512, 4096) == 0 and shim.tl_probe_due_host(_v(NOT_KNOWN), 2, 512, 4096) == 0
    assert shim.tl_probe_due_host(_v(NOT_KNOWN), 1, 511, 4096) == 0 and shim.tl_probe_due_host(_v(NOT_KNOWN), 1, 512, 4095) == 0
    assert shim.tl_probe_due_host(_v(NOT_KNOWN), 1, 1 << 40, 1 << 40) == 1
    for state, opt, wgs, tiles in itertools.product((0, 1, 2), (0, 1, 2, 3), (0, 511, 512, 513, 2605), (0, 4095, 4096, 4097, 31314)):
        assert shim.tl_probe_due_host(_v(state), opt, wgs, tiles) == probe_due(state, opt, wgs, tiles), (state, opt, wgs, tiles)


@pytest.mark.parametrize("given", [STREAMS, CALLER_ORDER])
def test_a_verdict_is_forgotten_at_the_sixteenth_repack_and_a_fresh_one_restarts_the_count(shim, given):
    v = _v()
    shim.tl_give_host(v, given)
    assert list(v) == [given, 0]
    for n in range(1, 16):
        shim.tl_repack_host(v)
        assert list(v) == [given, n]                   # ... not at the 15th
    shim.tl_repack_host(v)
    assert list(v) == [NOT_KNOWN, 0]                   # the 16th
    # a fresh verdict -- the same one again, or the other -- restarts the count
    shim.tl_give_host(v, given)
    for n in range(10):
        shim.tl_repack_host(v)
    shim.tl_give_host(v, given if given == STREAMS else STREAMS)
    assert v[1] == 0
    shim.tl_give_host(v, given)
    for n in range(15):
        shim.tl_repack_host(v)
    assert list(v) == [given, 15]
    shim.tl_repack_host(v)
    assert list(v) == [NOT_KNOWN, 0]
    # the whole walk against the restatement, unknown stretches included (they age too, and start over at 16)
    rng = np.random.default_rng(3)
    v, state, age = _v(), NOT_KNOWN, 0
    for step in range(400):
        if rng.random() < 0.05:
            state, age = int(rng.integers(1, 3)), 0
            shim.tl_give_host(v, state)
        else:
            state, age = repack(state, age)
            shim.tl_repack_host(v)
        assert list(v) == [state, age], step
