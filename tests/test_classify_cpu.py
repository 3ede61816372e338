"""Classification and DE groups (include/nabo_cluster.h, nabo_amd/_classify.py) without a GPU: the C header and its
symbols, argument checks, the no-device failure, the tests' plain restatement against the reference's results
(tests/golden/classify.npz, tools/gen_golden_classify.py), and the host logic with the device steps replaced by that
restatement."""
import os
import re
import subprocess

import numpy as np
import pytest

import nabo_amd
from nabo_amd import _lib

import _classify_ref as cref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_cluster_check(tmp_path):
    exe = os.path.join(str(tmp_path), "cluster_check")
    cmd = ["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(REPO, "include"),
           os.path.join(REPO, "tests", "abi_c", "cluster_check.c"), "-L" + os.path.join(REPO, "nabo_amd"), "-lnabo_knn",
           "-Wl,-rpath," + os.path.join(REPO, "nabo_amd"), "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0, r.stdout
    return exe


def test_header_is_plain_c_and_links(tmp_path):
    _lib.lib()
    exe = build_cluster_check(tmp_path)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0 and "%d entry points" % len(_lib.CLUSTER_SYMBOLS) in r.stdout, r.stdout


def test_library_exports_cluster_symbols():
    src = open(os.path.join(REPO, "include", "nabo_cluster.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = sorted(set(re.findall(r"\b(nabo_[a-z0-9_]+)\s*\(", src)))
    assert declared == sorted(_lib.CLUSTER_SYMBOLS)
    assert not set(_lib.CLUSTER_SYMBOLS) & (set(_lib.SYMBOLS) | set(_lib.GRAPH_SYMBOLS))
    L = _lib.lib()
    for n in _lib.CLUSTER_SYMBOLS:
        assert hasattr(L, n), n


def test_public_names():
    for n in ("classify_target", "classify_from_edges", "get_k_path_neighbours", "get_de_groups", "get_mapped_cells"):
        assert n in nabo_amd.__all__ and callable(getattr(nabo_amd, n))
    for n in ("k_path_neighbours", "set_de_groups"):
        assert callable(getattr(nabo_amd.RefGraph, n))


@pytest.mark.parametrize("rc, ptr, nbr, w, ncl", [
    ([0, 1], [0, 2, 1], [0, 1], [1.0, 1.0], 2),          # ptr not monotone
    ([0, 1], [1, 2], [0, 1], [1.0, 1.0], 2),             # ptr[0] != 0
    ([0, 1], [0, 2], [0, 2], [1.0, 1.0], 2),             # neighbour out of range
    ([0, 1], [0, 2], [-1, 0], [1.0, 1.0], 2),            # negative neighbour
    ([0, 2], [0, 2], [0, 1], [1.0, 1.0], 2),             # cluster id out of range
    ([0, -2], [0, 2], [0, 1], [1.0, 1.0], 2),            # cluster id below -1
    ([0, 0], [0, 2], [0, 1], [1.0, 1.0], 0),             # no cluster at all
])
def test_bad_rows_are_refused_before_any_device(rc, ptr, nbr, w, ncl):
    with pytest.raises(ValueError):
        nabo_amd.classify_from_edges(rc, ptr, nbr, w, n_clusters=ncl)


def test_null_outputs_and_null_graph_are_refused():
    import ctypes as C
    L = _lib.lib()
    ptr = np.array([0, 1], dtype=np.int64)
    nbr = np.array([0], dtype=np.int64)
    w = np.array([1.0])
    rc = np.array([0], dtype=np.int32)
    st = L.nabo_classify_targets(0, 1, rc.ctypes.data, 1, 1, ptr.ctypes.data, nbr.ctypes.data, w.ctypes.data, 0.5, 2, 0.1,
                                 None, None, None, None)
    assert st == _lib.E_INVALID and b"out_label" in L.nabo_last_error()
    assert L.nabo_refgraph_set_levels(None, 0, ptr.ctypes.data, None, -1, None) == _lib.E_INVALID
    assert L.nabo_cluster_last_device_ms(None) == _lib.E_INVALID
    ms = (C.c_double * 2)()
    assert L.nabo_cluster_last_device_ms(ms) == 0


def test_no_device_is_a_loud_failure():
    if nabo_amd.device_count() > 0:
        pytest.skip("a GPU is visible here; the no-device path is covered on the CPU box")
    with pytest.raises(nabo_amd.NaboError) as e:
        nabo_amd.classify_from_edges([0, 1], [0, 2], [0, 1], [1.0, 1.0])
    assert "no HIP device" in str(e.value)
    # the set-levels call needs a resident graph, whose creation fails the same way
    with pytest.raises(nabo_amd.NaboError) as e:
        from nabo_amd._paths import _DeviceGraph
        _DeviceGraph([0, 1, 1], [1]).set_levels([0, 1], [0])
    assert "no HIP device" in str(e.value)


def test_restatement_and_host_logic_reproduce_fixture_goldens(golden):
    assert cref.check_fixtures(golden("paths"), golden("classify"), cref.classify, cref.levels_step) >= 150


def test_restatement_and_host_logic_reproduce_quirk_goldens(golden):
    assert cref.check_quirks(golden("classify"), cref.classify, cref.levels_step) >= 250


def test_restatement_edges():
    """the restatement itself on rows whose answers are known by hand"""
    rc = [0, 0, 1, -1]
    ptr = [0, 3, 3, 5, 6]
    nbr = [0, 2, 0, 2, 3, 1]
    w = [0.25, 0.5, 0.75, 0.1, 0.9, 0.9]
    lab, best, tot, cnt, tied = cref.classify(rc, 2, ptr, nbr, w, 0.5, 2, 0.1, details=True)
    assert lab.tolist() == [0, -1, -1, -1] and best.tolist() == [0.75, 0.0, 0.0, 0.9] and tot.tolist() == [1.25, 0.0, 1.0, 0.9]
    assert cnt.tolist() == [1, 0, 3] and not tied.any()


def test_row_longer_than_the_limit_is_refused_before_any_device():
    """one lane walks a row with O(len^2) reads: the ABI takes at most 4096 edges per target node"""
    n = 4097
    with pytest.raises(ValueError) as e:
        nabo_amd.classify_from_edges([0, 1], [0, n], np.zeros(n, dtype=np.int64), np.ones(n), n_clusters=2)
    assert "at most 4096" in str(e.value)
