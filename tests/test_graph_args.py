"""What the C ABI answers to a malformed graph argument, through ctypes: NABO_E_INVALID with the message that names the
fault, found before any device is asked for (so never NABO_E_NODEVICE, with or without a GPU).  The texts are the
contract of nabo_layout_create, nabo_community_create, nabo_potential_create and nabo_umap_set_graph.

The three constructors are checked without a device.  nabo_umap_set_graph takes a handle, and nabo_umap_create needs a
device to make one, so its cases are the one GPU test here; they ask the same thing."""
import ctypes as C

import numpy as np
import pytest

from nabo_amd import _lib

N = 4
NAN = float("nan")
GOOD = dict(ptr=[0, 2, 3, 4, 4], nbr=[1, 2, 0, 0], w=[0.5, 0.25, 0.5, 0.25])

# the fault -> (what is changed, the message of a constructor, the message of nabo_umap_set_graph)
FAULTS = {
    "null_ptr": (dict(ptr=None), "ptr is NULL", "NULL argument"),
    "ptr0_is_1": (dict(ptr=[1, 2, 3, 4, 4]), "ptr[0] = 1, must be 0", "ptr[0] = 1, must be 0"),
    "ptr_falls": (dict(ptr=[0, 2, 1, 4, 4]), "ptr is not monotone at node 1", "ptr is not monotone at node 1"),
    "nbr_is_n": (dict(nbr=[1, 2, 4, 0]), "nbr[2] = 4 is not a node in [0, 4)", "nbr[2] = 4 is not another node in [0, 4)"),
    "nbr_is_minus_1": (dict(nbr=[1, -1, 0, 0]), "nbr[1] = -1 is not a node in [0, 4)", "nbr[1] = -1 is not another node in [0, 4)"),
    "null_nbr": (dict(nbr=None), {"layout": "nbr or w is NULL", "community": "nbr or w is NULL", "potential": "nbr is NULL"},
                 "the graph has no arc, or nbr or w is NULL"),
    "nan_weight": (dict(w=[0.5, 0.25, NAN, 0.25]), {"layout": "w[2] is not finite", "community": "w[2] is negative or not finite"},
                   "w[2] is not finite and positive"),
    "negative_weight": (dict(w=[0.5, 0.25, 0.5, -0.25]), {"community": "w[3] is negative or not finite"}, None),
}


def _arrays(change):
    a = dict(GOOD, **change)
    keep = {"ptr": None if a["ptr"] is None else np.array(a["ptr"], dtype=np.int64),
            "nbr": None if a["nbr"] is None else np.array(a["nbr"], dtype=np.int64),
            "w": None if a["w"] is None else np.array(a["w"], dtype=np.float64)}
    return keep, {k: None if v is None else v.ctypes.data for k, v in keep.items()}


def _answer(rc):
    return rc, _lib.lib().nabo_last_error().decode("utf-8")


def _constructor_cases():
    for fault, (_, want, _) in sorted(FAULTS.items()):
        for step in ("layout", "community", "potential"):
            text = want.get(step) if isinstance(want, dict) else want
            if text is not None:                       # the potential takes no weights, only the clustering minds a sign
                yield pytest.param(step, fault, text, id="%s-%s" % (step, fault))


@pytest.mark.parametrize("step,fault,want", list(_constructor_cases()))
def test_constructor_names_the_fault_before_it_asks_for_a_device(step, fault, want):
    change = FAULTS[fault][0]
    keep, p = _arrays(change)
    L, h = _lib.lib(), C.c_void_p()
    if step == "layout":
        rc = L.nabo_layout_create(C.byref(h), 0, N, p["ptr"], p["nbr"], p["w"])
    elif step == "community":
        rc = L.nabo_community_create(C.byref(h), 0, N, p["ptr"], p["nbr"], p["w"], 10000.0)
    else:
        rc = L.nabo_potential_create(C.byref(h), 0, N, p["ptr"], p["nbr"])
    assert _answer(rc) == (_lib.E_INVALID, want) and not h.value
    del keep


@pytest.mark.gpu
@pytest.mark.parametrize("fault", sorted(k for k, v in FAULTS.items() if v[2] is not None))
def test_umap_set_graph_names_the_fault(fault):
    change, _, want = FAULTS[fault]
    keep, p = _arrays(change)
    L, h = _lib.lib(), C.c_void_p()
    _lib.check(L.nabo_umap_create(C.byref(h), 0, N, 2))
    try:
        assert _answer(L.nabo_umap_set_graph(h, p["ptr"], p["nbr"], p["w"])) == (_lib.E_INVALID, want)
    finally:
        L.nabo_umap_destroy(h)
    del keep
