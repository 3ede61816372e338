"""Hop distances on the reference graph (include/nabo_graph.h, nabo_amd/_paths.py) without a GPU: the C header and
its symbols, argument checks, the no-device failure, and the tests' own BFS oracle against the reference's results
(tests/golden/paths.npz, tools/gen_golden_paths.py)."""
import json
import os
import subprocess

import numpy as np
import pytest

import nabo_amd
from nabo_amd import _lib

import _paths_oracle as orc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_is_plain_c_and_links(tmp_path):
    _lib.lib()
    exe = os.path.join(str(tmp_path), "paths_check")
    cmd = ["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(REPO, "include"),
           os.path.join(REPO, "tests", "abi_c", "paths_check.c"), "-L" + os.path.join(REPO, "nabo_amd"), "-lnabo_knn",
           "-Wl,-rpath," + os.path.join(REPO, "nabo_amd"), "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0 and "%d entry points" % len(_lib.GRAPH_SYMBOLS) in r.stdout, r.stdout


def test_library_exports_graph_symbols():
    import re
    src = open(os.path.join(REPO, "include", "nabo_graph.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = sorted(set(re.findall(r"\b(nabo_[a-z0-9_]+)\s*\(", src)))
    assert declared == sorted(_lib.GRAPH_SYMBOLS)
    assert not set(_lib.GRAPH_SYMBOLS) & set(_lib.SYMBOLS)
    L = _lib.lib()
    for n in _lib.GRAPH_SYMBOLS:
        assert hasattr(L, n), n


@pytest.mark.parametrize("ptr, nbr", [
    ([1, 2], [0, 0]),                 # ptr[0] != 0
    ([0, 2, 1], [0, 1]),              # not monotone
    ([0, 1, 2], [0, 2]),              # neighbour out of range
    ([0, 1, 2], [-1, 0]),             # negative neighbour
])
def test_bad_csr_is_refused(ptr, nbr):
    with pytest.raises(ValueError):
        nabo_amd.group_hops(ptr, nbr, [0, 2], [0, 1])


def test_no_device_is_a_loud_failure():
    if nabo_amd.device_count() > 0:
        pytest.skip("a GPU is visible here; the no-device path is covered on the CPU box")
    with pytest.raises(nabo_amd.NaboError) as e:
        nabo_amd.group_hops([0, 1, 1], [1], [0, 2], [0, 1])
    assert "no HIP device" in str(e.value)


def _fixture_graph(d, tag):
    ref = [str(x) for x in d[tag + "_ref_nodes"]]
    uptr, ucol = orc.undirected(len(ref), d[tag + "_ref_ptr"], d[tag + "_ref_nbr"])
    return ref, uptr, ucol


def test_oracle_agrees_with_reference_fixture(golden):
    d = golden("paths")
    for tag, t in (("small", "ME"), ("small", "IG"), ("c1", "ME")):
        ref, uptr, ucol = _fixture_graph(d, tag)
        p = "%s_%s" % (tag, t)
        tp, tn = d[p + "_t_ptr"], d[p + "_t_nbr"]
        if tag == "c1":                      # the whole c1 target takes minutes in Python: every 10th node
            sel = np.arange(0, len(tp) - 1, 10)
            rows = [tn[tp[i]:tp[i + 1]] for i in sel]
            tp = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
            tn = np.concatenate(rows)
            want = d[p + "_spec_nofill"][sel]
        else:
            want = d[p + "_spec_nofill"]
        got = np.array(orc.specificity(uptr, ucol, tp, tn, fill_na=False))
        assert np.array_equal(got, want, equal_nan=True), p
        if tag != "c1":
            assert np.array_equal(np.array(orc.specificity(uptr, ucol, tp, tn, fill_na=True)), d[p + "_spec_fill"],
                                  equal_nan=True), p
        for nodes, v in zip(json.loads(str(d[p + "_cspl_lists"])), d[p + "_cspl_vals"]):
            hops = [int(orc.bfs(uptr, ucol, a, [b])[b]) for a, b in zip(nodes[:-1], nodes[1:])]
            assert (float(np.mean(hops)) if hops else float("nan")) == v or (v != v and not hops), (p, nodes)


def test_ref_specificity_matches_fixture_without_gpu(golden):
    """host code only: the reference's get_ref_specificity from the target's rows and the recorded specificity"""
    from nabo_amd._paths import _ref_specificity_rows
    d = golden("paths")
    for tag, t in (("small", "ME"), ("small", "IG"), ("c1", "ME")):
        ref = [str(x) for x in d[tag + "_ref_nodes"]]
        pos = {n: i for i, n in enumerate(ref)}
        p = "%s_%s" % (tag, t)
        t_nodes = [str(x) for x in d[p + "_t_nodes"]]
        vals = dict(zip(t_nodes, d[p + "_spec_fill"].tolist()))
        for incl, q in ((False, "_refspec"), (True, "_refspec_incl")):
            got = _ref_specificity_rows(ref, pos, len(ref), t_nodes, d[p + "_t_ptr"], d[p + "_t_nbr"], vals, incl)
            assert list(got) == [str(x) for x in d[p + q + "_nodes"]], p
            assert np.array_equal(np.array([float(v) for v in got.values()]), d[p + q + "_vals"], equal_nan=True), p
