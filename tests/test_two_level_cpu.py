"""The two-level slot order of the one-product operands without a GPU: nabo_amd/csrc/l2c_slots.h, compiled here with g++
through tests/two_level_host, against a plain restatement -- the map is a bijection for every eligible g, the first step of
32 slots holds exactly 28 components and the four special slots, and in float64 on random f16 vectors the first step's
sum never exceeds the full score while the two tail products cancel exactly."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAIL, NH, NL, EY, TAIL2, ZERO = -1, -2, -3, -4, -5, -6


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("l2c_slots") / "libl2c_slots_host.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-shared", "-fPIC", "-I" + os.path.join(REPO, "nabo_amd", "csrc"),
                           os.path.join(REPO, "tests", "two_level_host", "slots_shim.cpp"), "-o", so])
    lib = C.CDLL(so)
    lib.l2c_round_up_host.restype = C.c_float
    lib.l2c_round_up_host.argtypes = [C.c_double]
    return lib


def test_eligible_g(L):
    assert [g for g in range(1, 130) if L.l2c_slots_fit_host(g)] == list(range(29, 60))


@pytest.mark.parametrize("g", range(29, 60))
def test_the_slot_map_is_a_bijection_and_step_0_is_28_components_and_four_slots(L, g):
    holds = [L.l2c_slot_holds_host(g, p) for p in range(64)]
    comps = [h for h in holds if h >= 0]
    assert sorted(comps) == list(range(g)), "every component in exactly one slot"
    assert [L.l2c_slot_of_comp_host(e) for e in range(g)] == [holds.index(e) for e in range(g)]
    for special in (TAIL, NH, NL, EY, TAIL2):
        assert holds.count(special) == 1
    assert holds.count(ZERO) == 64 - g - 5
    assert holds[:28] == list(range(28)) and holds[28:32] == [TAIL, NH, NL, EY]          # step 0
    assert all(h >= 28 or h in (TAIL2, ZERO) for h in holds[32:])                           # step 1
    assert holds[L.l2c_slot_tail2_host(g)] == TAIL2 and L.l2c_norm_slot_host(g, 1) == holds.index(NH)
    assert L.l2c_norm_slot_host(g, 0) == g
    assert [bool(L.l2c_slot_is_comp_host(g, p, 1)) for p in range(64)] == [h >= 0 for h in holds]
    assert [bool(L.l2c_slot_is_comp_host(g, p, 0)) for p in range(64)] == [p < g for p in range(64)]


def _up(L, v):
    """an f16 that is no smaller than v: the header's factor, then round to nearest"""
    return float(np.float16(L.l2c_round_up_host(float(v))))


@pytest.mark.parametrize("g", [29, 37, 50, 59])
def test_the_first_step_is_a_lower_bound_and_the_tails_cancel(L, g):
    rng = np.random.default_rng(g)
    for scale in (1e-3, 1.0, 300.0):
        X = (rng.standard_normal((200, g)) * scale).astype(np.float16).astype(np.float64)       # hi parts of targets
        Y = (rng.standard_normal((200, g)) * scale).astype(np.float16).astype(np.float64)       # ... and references
        for x, y in zip(X, Y):
            tx2, ty = _up(L, np.sqrt((x[28:] ** 2).sum())), _up(L, np.sqrt((y[28:] ** 2).sum()))
            assert tx2 >= np.sqrt((x[28:] ** 2).sum()) and ty >= np.sqrt((y[28:] ** 2).sum())
            ref = np.zeros(64)
            tgt = np.zeros(64)
            for p in range(64):
                h = L.l2c_slot_holds_host(g, p)
                if h >= 0:
                    ref[p], tgt[p] = y[h], -2.0 * x[h]
                elif h == TAIL:
                    ref[p], tgt[p] = ty, -2.0 * tx2
                elif h == TAIL2:
                    ref[p], tgt[p] = ty, 2.0 * tx2
            prod = ref * tgt                                           # the norm and error slots add the same to both sums
            lb1, full = prod[:32].sum(), -2.0 * float(x @ y)
            assert prod[28] + prod[L.l2c_slot_tail2_host(g)] == 0.0, "the two tail products cancel exactly"
            assert abs(prod.sum() - full) <= 1e-9 * (1.0 + abs(full))
            assert lb1 <= full + 1e-9 * (1.0 + abs(full)), (g, scale, lb1, full)
