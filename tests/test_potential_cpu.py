"""The differentiation potential (include/nabo_potential.h, nabo_amd/_potential.py) without a GPU: the C header and its
symbols, the argument checks, and the tests' numpy restatement (tests/_potential_ref.py) against the dense route -- a
pinv it takes itself, the pinv and the reference's own calc_diff_potential as recorded in tests/golden/potential.npz."""
import os
import re
import subprocess
import warnings

import numpy as np
import pytest

import nabo_amd
from nabo_amd import _lib, _potential

import _potential_ref as pr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAGS = ("ones", "r")


@pytest.fixture(scope="module")
def gold(golden):
    return golden("potential")


def graph_names():
    return [str(x) for x in np.load(os.path.join(REPO, "tests", "golden", "potential.npz"))["names"]]


def test_public_names_and_symbols():
    for n in ("diff_potential_csr", "Potential", "calc_diff_potential"):
        assert n in nabo_amd.__all__ and callable(getattr(nabo_amd, n))
    assert callable(nabo_amd.RefGraph.calc_diff_potential)
    src = open(os.path.join(REPO, "include", "nabo_potential.h")).read()
    assert '#include "nabo_knn.h"' in src and "nabo_potential.h" not in open(os.path.join(REPO, "include", "nabo_knn.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert sorted(set(re.findall(r"\b(nabo_[a-z0-9_]+)\s*\(", src))) == sorted(_lib.POTENTIAL_SYMBOLS)
    others = (_lib.SYMBOLS + _lib.GRAPH_SYMBOLS + _lib.CLUSTER_SYMBOLS + _lib.DE_SYMBOLS + _lib.PCA_SYMBOLS + _lib.PCA_FIT_SYMBOLS
              + _lib.QC_SYMBOLS + _lib.LAYOUT_SYMBOLS + _lib.UMAP_SYMBOLS + _lib.COMMUNITY_SYMBOLS)
    assert not set(_lib.POTENTIAL_SYMBOLS) & set(others)
    L = _lib.lib()
    for n in _lib.POTENTIAL_SYMBOLS:
        assert hasattr(L, n), n


def test_geometry_needs_no_device(gold):
    group, thr, rows = _potential.geometry()
    assert group in (1, 2, 4, 8, 16, 32, 64) and group <= thr and rows % 256 == 0 and rows >= 256
    hip = open(os.path.join(REPO, "nabo_amd", "csrc", "potential.hip")).read()
    assert "PT_GROUP = %d;" % group in hip and "PT_LONG = %d;" % thr in hip and "PT_ROWS = %d;" % rows in hip
    # the golden file's hub and path graphs were cut for this geometry
    assert (int(gold["long_threshold"]), int(gold["block_rows"])) == (thr, rows), "run tools/gen_golden_potential.py"
    assert "path%d" % (rows - 1) in graph_names() and "path%d" % (rows + 1) in graph_names()


def test_header_is_plain_c_and_links(tmp_path):
    _lib.lib()
    exe = os.path.join(str(tmp_path), "potential_check")
    cmd = ["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(REPO, "include"),
           os.path.join(REPO, "tests", "abi_c", "potential_check.c"), "-L" + os.path.join(REPO, "nabo_amd"), "-lnabo_knn",
           "-Wl,-rpath," + os.path.join(REPO, "nabo_amd"), "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0 and "%d entry points" % len(_lib.POTENTIAL_SYMBOLS) in r.stdout, r.stdout


GOOD = dict(ptr=[0, 1, 2, 3], nbr=[1, 2, 0])


@pytest.mark.parametrize("change", [
    {"ptr": [0, 1, 2]},                                      # does not end at len(nbr)
    {"ptr": [1, 1, 2, 3]},
    {"ptr": [0, 2, 1, 3]},                                   # not monotone
    {"ptr": [0]},                                            # no node
    {"ptr": [[0, 1, 2, 3]]},                                 # not 1-D
    {"nbr": [1, 2, 3]},                                      # no such node
    {"nbr": [1, 2, -1]},
    {"ptr": [0, 1, 2, 2, 2], "nbr": [1, 0]},                 # nodes 2 and 3 have no edge
    {"ptr": [0, 0, 1], "nbr": [1]},                          # node 0 has no edge: a self-loop of 1 does not reach it
    {"r": [1.0, 2.0]},                                       # another length than the graph
    {"r": [1.0, np.nan, 1.0]},
    {"r": [1.0, np.inf, 1.0]},
    {"r": ["a", "b", "c"]},
    {"tol": -1e-3},
    {"tol": np.nan},
    {"tol": np.inf},
    {"tol": "tight"},
    {"max_iter": 0},
    {"max_iter": 2.5},
    {"max_iter": True},
])
def test_bad_arguments_raise_before_any_device(change):
    with pytest.raises(ValueError) as e:
        nabo_amd.diff_potential_csr(**dict(GOOD, **change))
    assert str(e.value).startswith("ERROR: ")


def test_no_device_is_a_loud_failure():
    if nabo_amd.device_count() > 0:
        pytest.skip("a GPU is visible here; the no-device path is covered on the CPU box")
    with pytest.raises(nabo_amd.NaboError) as e:
        nabo_amd.diff_potential_csr(**GOOD)
    assert "no HIP device" in str(e.value)


def test_simple_graph_degrees_and_components():
    # (0, 1) listed three times from both ends, loops on 1 and 4, 4 alone with its loop, 2 - 3 apart from 0 - 1
    ptr, nbr = pr.csr_of_edges(5, [(0, 1), (1, 0), (1, 1), (0, 1), (2, 3), (4, 4), (1, 1)])
    G = pr.Graph(ptr, nbr)
    assert G.d.tolist() == [1, 2, 1, 1, 1] and G.c.tolist() == [1, 1, 1, 1, 0] and G.loop.tolist() == [0, 1, 0, 0, 1]
    assert G.label.tolist() == [0, 0, 2, 2, 4] and G.size.tolist() == [2, 2, 1]
    assert list(zip(G.src.tolist(), G.dst.tolist())) == [(0, 1), (1, 0), (2, 3), (3, 2)]
    b = pr.rhs(G, [3.0, -1.0, 2.0, 5.0, 7.0])
    assert np.abs(G.comp_sum(b)).max() <= 8 * pr.U * np.abs(b).max()      # consistent: b sums to 0 over each component
    assert b[4] == 0.0                                                    # a lone looped node: r' = r - d (d r / d^2) = 0


@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("name", ["blob96", "hub", "path257", "one_loop", "pair", "loop_beside_clique", "mapping_small"])
def test_yardstick_against_a_dense_pinv_taken_here(gold, name, tag):
    """V = pinv(I - A/D) r is what the header's five steps give: K e = rho for the error e of the centred iterate, so
    ||e|| <= ||rho|| / lambda_2; the pinv's own rounding is the golden file's measured delta"""
    ptr, nbr = gold[name + "_ptr"], gold[name + "_nbr"]
    r = None if tag == "ones" else gold[name + "_r"]
    G = pr.Graph(ptr, nbr)
    b = pr.rhs(G, r)
    s = pr.PCG(G, b, 1e-10, 10000).run()
    V = pr.centre(G, s.x)
    pinv = pr.pinv_potential(G, r)
    lam2 = pr.lambda2(G)
    assert abs(lam2 - float(gold[name + "_lambda2"])) <= 1e-9 * lam2 or lam2 == float(gold[name + "_lambda2"])
    rho = np.linalg.norm(b - G.product(s.x))
    bound = rho / lam2 + 4.0 * float(gold["%s_%s_delta_pinv" % (name, tag)])
    err = np.linalg.norm(V - pinv)
    print("%s %s: %d iterations, ||V - pinv|| = %.3g, bound %.3g" % (name, tag, s.it, err, bound))
    assert s.status == pr.CONVERGED and err <= bound


@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("name", graph_names())
def test_yardstick_against_the_golden_values(gold, name, tag):
    """every graph of the tests converges at tol = 1e-10, in the iterations recorded, to the recorded pinv and to the
    reference's own calc_diff_potential within the derived bound"""
    ptr, nbr = gold[name + "_ptr"], gold[name + "_nbr"]
    r = None if tag == "ones" else gold[name + "_r"]
    key = "%s_%s_" % (name, tag)
    G = pr.Graph(ptr, nbr)
    b = pr.rhs(G, r)
    s = pr.PCG(G, b, 1e-10, 10000).run()
    V = pr.centre(G, s.x)
    assert s.status == pr.CONVERGED and s.it == int(gold[key + "iterations"]), "the yardstick changed: run tools/gen_golden_potential.py"
    first = np.linalg.norm(b - G.product(s.x)) / float(gold[name + "_lambda2"])
    for what in ("pinv", "ref"):
        err, bound = np.linalg.norm(V - gold[key + what]), first + 4.0 * float(gold[key + "delta_" + what])
        print("%s %s: ||V - %s|| = %.3g, bound %.3g" % (name, tag, what, err, bound))
        assert err <= bound
    # minimum norm: mean 0 per component (the mean is good to n u sum |x| / n, the sum of V to n u sum |V|)
    assert np.abs(G.comp_sum(V)).max() <= 2 * G.n * pr.U * (np.abs(s.x).sum() + np.abs(V).sum())
    if s.bnorm == 0.0:
        assert s.it == 0 and not V.any()


def test_stopping_rule_of_the_yardstick(gold):
    ptr, nbr = gold["path257_ptr"], gold["path257_nbr"]
    G = pr.Graph(ptr, nbr)
    b = pr.rhs(G, gold["path257_r"])
    s = pr.PCG(G, b, 1e-10, 10).run()
    assert s.status == pr.MAX_ITER and s.it == 10 and s.true_residual() > 1e-3
    assert s.step() and s.it == 10                                       # a stopped run stays where it is
    # r proportional to d: b = 0, no iteration
    z = pr.PCG(G, pr.rhs(G, 2.5 * G.d), 1e-10, 10)
    assert z.status == pr.CONVERGED and z.it == 0 and z.bnorm == 0.0
    # a direction in the null space is a breakdown, not a NaN
    k = pr.PCG(G, b, 1e-10, 10)
    k.p = np.ones(G.n)
    assert k.step() and k.status == pr.BREAKDOWN and np.isfinite(k.x).all() and k.it == 0


def test_dict_by_node_name_and_the_reference_quirk(monkeypatch, capsys):
    ref_nodes = ["c%d_WT" % i for i in (2, 0, 1)]
    pos = {"c0_WT": 0, "c1_WT": 1, "c2_WT": 2}
    seen = {}

    def solve(ptr, nbr, r, tol, max_iter, device):
        seen.update(r=None if r is None else r.tolist(), tol=tol, max_iter=max_iter, device=device)
        return np.array([0.5, -0.25, -0.25]), {"status": "converged"}

    monkeypatch.setattr(_potential, "diff_potential_csr", solve)
    V = _potential._potential_of_graph(ref_nodes, pos, [0, 1, 2, 2], [1, 2], None, 1e-9, 50, 0)
    assert V == {"c2_WT": -0.25, "c0_WT": 0.5, "c1_WT": -0.25} and list(V) == ref_nodes
    assert seen == dict(r=None, tol=1e-9, max_iter=50, device=0)
    V = _potential._potential_of_graph(ref_nodes, pos, [0, 1, 2, 2], [1, 2], {"c0_WT": 3, "c1_WT": -1.5, "c2_WT": 2, "other": 9}, 1e-9, 50, 0)
    assert seen["r"] == [3.0, -1.5, 2.0] and list(V) == ref_nodes
    # a node missing from r: the reference prints its line (the %s never filled in) and returns {}
    capsys.readouterr()
    assert _potential._potential_of_graph(ref_nodes, pos, [0, 1, 2, 2], [1, 2], {"c0_WT": 3, "c2_WT": 2}, 1e-9, 50, 0) == {}
    assert capsys.readouterr().out == "ERROR: %s node is missing in r\n"
    with pytest.raises(ValueError):
        _potential._potential_of_graph(ref_nodes, pos, [0, 1, 2, 2], [1, 2], {"c0_WT": 3, "c1_WT": np.nan, "c2_WT": 2}, 1e-9, 50, 0)
    with pytest.raises(ValueError):                                        # c2 has no edge: before any device
        _potential._potential_of_graph(ref_nodes, pos, [0, 1, 2, 2], [1, 0], None, 1e-9, 50, 0)


def test_a_run_that_does_not_converge_warns(monkeypatch):
    class Fake:
        def __init__(self, *a):
            pass

        def __enter__(self):
            return self

        def __exit__(self, *exc):
            pass

        def solve(self, r):
            return np.zeros(3), {"status": Fake.status, "iterations": 10, "true_residual": 0.125}

    monkeypatch.setattr(_potential, "Potential", Fake)
    for status in ("max_iter", "breakdown"):
        Fake.status = status
        with pytest.warns(RuntimeWarning, match="0.125") as rec:
            V, info = _potential.diff_potential_csr(**GOOD)
        assert status in str(rec[0].message) and info["status"] == status and V.shape == (3,)
    Fake.status = "converged"
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        _potential.diff_potential_csr(**GOOD)
