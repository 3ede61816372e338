"""The agglomeration step (include/nabo_agglom.h, nabo_amd._community) without a GPU: the C header and its symbols, the
argument checks, and the tests' numpy / Python-int restatement (tests/_agglom_ref.py) held to the definition it restates --
the passes give the sequential greedy matching, every pass with a candidate matches a pair, the path of Q is the Q of the
cut at every step -- and to what tests/golden/agglom.npz recorded of it on the golden graph."""
import os
import re
import subprocess

import numpy as np
import pytest

import nabo_amd
from nabo_amd import _lib

import _agglom_ref as ar
import _community_ref as cr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOOD = dict(ptr=[0, 1, 2, 3], nbr=[1, 2, 0], w=[0.5, 0.25, 1.0])


def test_public_names_and_symbols():
    for n in ("agglomerate_csr", "make_clusters"):
        assert n in nabo_amd.__all__ and callable(getattr(nabo_amd, n))
    for n in ("agglomerate", "dendrogram", "cut", "match_pass", "match", "agglom_ms"):
        assert callable(getattr(nabo_amd.Community, n))
    assert callable(nabo_amd.RefGraph.make_clusters)
    src = open(os.path.join(REPO, "include", "nabo_agglom.h")).read()
    assert '#include "nabo_community.h"' in src
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert sorted(set(re.findall(r"\b(nabo_[a-z0-9_]+)\s*\(", src))) == sorted(_lib.AGGLOM_SYMBOLS)
    others = (_lib.SYMBOLS + _lib.GRAPH_SYMBOLS + _lib.CLUSTER_SYMBOLS + _lib.DE_SYMBOLS + _lib.PCA_SYMBOLS + _lib.PCA_FIT_SYMBOLS
              + _lib.QC_SYMBOLS + _lib.LAYOUT_SYMBOLS + _lib.UMAP_SYMBOLS + _lib.UMAP_TRANSFORM_SYMBOLS + _lib.COMMUNITY_SYMBOLS
              + _lib.POTENTIAL_SYMBOLS)
    assert not set(_lib.AGGLOM_SYMBOLS) & set(others)
    L = _lib.lib()
    for n in _lib.AGGLOM_SYMBOLS:
        assert hasattr(L, n), n
    # the pass shares the sweep's row geometry
    hip = open(os.path.join(REPO, "nabo_amd", "csrc", "agglom.hip")).read()
    assert "AG_GROUP = %d;" % nabo_amd._community.geometry()[0] in hip


def test_header_is_plain_c_and_links(tmp_path):
    _lib.lib()
    exe = os.path.join(str(tmp_path), "agglom_check")
    cmd = ["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(REPO, "include"),
           os.path.join(REPO, "tests", "abi_c", "agglom_check.c"), "-L" + os.path.join(REPO, "nabo_amd"), "-lnabo_knn",
           "-Wl,-rpath," + os.path.join(REPO, "nabo_amd"), "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0 and "%d entry points" % len(_lib.AGGLOM_SYMBOLS) in r.stdout, r.stdout


@pytest.mark.parametrize("change", [{"n_clusters": 0}, {"n_clusters": -3}, {"n_clusters": 2.0}, {"n_clusters": True}, {"w": [0.5, -0.25, 1.0]},
                                    {"nbr": [1, 2, 3]}, {"weight_scale": 0}])
def test_bad_arguments_raise_before_any_device(change):
    with pytest.raises(ValueError) as e:
        nabo_amd.agglomerate_csr(**dict(GOOD, **change))
    assert str(e.value).startswith("ERROR: ")


def test_no_device_is_a_loud_failure():
    if nabo_amd.device_count() > 0:
        pytest.skip("a GPU is visible here; the no-device path is covered on the CPU box")
    with pytest.raises(nabo_amd.NaboError) as e:
        nabo_amd.agglomerate_csr(**GOOD)
    assert "no HIP device" in str(e.value)


def random_graph(rng, n, edges, weights):
    """few distinct weights, so that many gains are equal and the ids decide"""
    es = {}
    for _ in range(edges):
        i, j = rng.integers(0, n, size=2).tolist()
        es[(min(i, j), max(i, j))] = float(rng.choice(weights))          # self-loops included
    return cr.csr_of_edges(n, [(i, j, x) for (i, j), x in es.items()])


def levels_of(ptr, nbr, w, n_min=1):
    levels = []
    res = ar.run(ptr, nbr, w, n_min=n_min, levels=levels)
    return res, levels


def test_the_passes_give_the_sequential_greedy_matching():
    rng = np.random.default_rng(0)
    seen_ties = rounds = 0
    cases = [random_graph(rng, int(rng.integers(2, 40)), int(rng.integers(1, 120)), [1.0, 1.0, 0.5, 0.25]) for _ in range(60)]
    cases += list(cr.tiny_graphs().values())
    for ptr, nbr, w in cases:
        res, levels = levels_of(ptr, nbr, w)
        for lv, pairs, passes in levels:                    # level 0 and every coarse level the run meets
            greedy = ar.greedy_matching(lv, res["two_m"])
            if greedy:
                assert pairs == greedy
                gains = [p[2] for p in pairs]
                assert gains == sorted(gains, reverse=True) and min(gains) > 0
                seen_ties += len(set(gains)) < len(gains)
            else:                                           # no positive gain: the single first pair of the order
                assert pairs == [ar.first_pair(lv, res["two_m"])] and pairs[0][2] <= 0
            ends = [x for c, d, _, _ in pairs for x in (c, d)]
            assert len(set(ends)) == len(ends) and all(c < d for c, d, _, _ in pairs)
            rounds += 1
    assert seen_ties > 20 and rounds > 200


def test_every_pass_with_a_candidate_matches_a_pair():
    rng = np.random.default_rng(1)
    with_candidates = 0
    for _ in range(40):
        ptr, nbr, w = random_graph(rng, int(rng.integers(2, 50)), int(rng.integers(1, 150)), [1.0, 0.5])
        res, levels = levels_of(ptr, nbr, w)
        for lv, pairs, passes in levels:
            _, p, trace = ar.match(lv, res["two_m"])
            assert p == passes == len(trace) and trace[-1][1] == 0
            for picked, matched in trace:
                assert (matched >= 1) == (picked >= 1) and 2 * matched <= picked
                with_candidates += picked >= 1
            assert trace[-1] == (0, 0)                      # the last pass saw no candidate at all
    assert with_candidates > 150                            # the graphs did exercise the property


def test_a_pass_under_a_mask_leaves_the_others_alone():
    ptr, nbr, w = cr.tiny_graphs()["two_k4_bridge"]
    lv, two_m = cr.level0(ptr, nbr, w)
    free = np.array([1, 0, 1, 1, 1, 1, 0, 1], dtype=bool)
    partner, D, a = ar.match_pass(lv, two_m, free)
    assert partner[1] == -1 and partner[6] == -1 and D[1] == 0 and D[6] == 0
    assert all(free[p] for p in partner[partner >= 0].tolist()) and partner[0] == 2 and partner[2] == 0
    assert D[0] == 10000 * two_m - int(lv.k[0]) * int(lv.k[2]) and a[0] == 10000


def test_q_path_is_the_q_of_the_cut_at_every_step():
    rng = np.random.default_rng(2)
    for ptr, nbr, w in [random_graph(rng, 45, 110, [1.0, 0.5, 0.25, 0.07])] + list(cr.tiny_graphs().values()):
        res = ar.run(ptr, nbr, w)
        lv0, two_m, n0 = res["lv0"], res["two_m"], res["lv0"].n
        assert len(res["q_path"]) == len(res["merges"]) + 1 == n0 - res["n_end"] + 1
        for t in range(len(res["merges"]) + 1):
            labels, C, q = ar.cut(res, n0 - t)
            assert C == n0 - t and q == res["q_path"][t] == cr.label_q(lv0, two_m, labels, 1.0)
            # the exact integer is Q (2m)^2: sum_in 2m - sum_d2 of the same labels
            nx, _ = cr.aggregate(lv0, labels - 1)
            assert res["x_path"][t] == sum(nx.inn.tolist()) * two_m - sum(x * x for x in nx.k.tolist())
            assert np.array_equal(cr.finish(lv0, labels, True)[0], labels)                   # connected by construction
        # a merge changes Q by exactly 2 D / (2m)^2, and the peak is the earliest largest
        for t, (c, d, rnd, a, ka, kb) in enumerate(res["merges"].tolist()):
            assert res["x_path"][t + 1] - res["x_path"][t] == 2 * (a * two_m - ka * kb) and c < d
        assert res["peak"] == res["x_path"].index(max(res["x_path"])) and ar.cut(res, 0)[1] == n0 - res["peak"]
        assert (np.diff(res["merges"][:, 2]) >= 0).all()
        with pytest.raises(ValueError):
            ar.cut(res, res["n_end"] - 1 if res["n_end"] > 1 else n0 + 1)


def test_n_min_takes_the_prefix_of_the_round():
    ptr, nbr, w = random_graph(np.random.default_rng(3), 60, 200, [1.0, 0.5, 0.25])
    full = ar.run(ptr, nbr, w)
    first = int((full["merges"][:, 2] == 0).sum())
    assert first > 3
    res = ar.run(ptr, nbr, w, n_min=60 - (first - 2))
    assert res["rounds"] == 1 and res["n_end"] == 60 - (first - 2) and np.array_equal(res["merges"], full["merges"][:first - 2])
    assert ar.run(ptr, nbr, w, n_min=60)["merges"].shape == (0, 6)


def test_golden_graph_reproduces_the_recorded_run(golden):
    d, g = golden("community"), golden("agglom")
    res = ar.run(d["ptr"], d["nbr"].astype(np.int64), d["w"])
    assert (res["rounds"], res["passes"], res["peak"], res["n_end"]) == (int(g["rounds"]), int(g["passes"]), int(g["peak"]), int(g["n_end"])), \
        "the yardstick changed: run tools/gen_golden_agglom.py"
    assert (res["rounds"], res["passes"]) == (16, 65) and res["lv0"].n - res["peak"] == 8
    assert np.array_equal(res["merges"], g["merges"]) and res["q_path"][res["peak"]] == float(g["peak_q"]) == 0.6649862725562173
    # the peak is the Louvain yardstick's partition at resolution 1 and networkx's CNM peak, to every digit
    assert float(g["peak_q"]) == float(d["ref_q"][1]) == float(g["nx_peak_q"])
    for c, q, nq in zip(g["cuts"].tolist(), g["q_cut"].tolist(), g["nx_q"].tolist()):
        if c < res["n_end"]:                                # below the graph's 7 components: neither can get there
            assert np.isnan(q) and np.isnan(nq)
            with pytest.raises(ValueError):
                ar.cut(res, c)
            continue
        assert ar.cut(res, c)[2] == q
        print("%d clusters: Q = %.6f, networkx %s CNM: %.6f, apart by %+.6f" % (c, q, str(g["networkx_version"]), nq, q - nq))
    assert g["cuts"].tolist() == [5, 8, 10, 20, 40]
