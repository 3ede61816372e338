"""The clustering step (include/nabo_community.h, nabo_amd/_community.py) without a GPU: the C header and its symbols, the
argument checks, the quantiser, the tests' numpy restatement (tests/_community_ref.py) on tiny graphs whose answer is
known, its invariants, its quality against networkx's Louvain as recorded in tests/golden/community.npz, the writers and
the no-device failure."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import nabo_amd
from nabo_amd import _community, _lib

import _community_ref as cr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = cr.tiny_graphs()


@pytest.fixture(scope="module")
def gold(golden):
    return golden("community")


def test_public_names_and_symbols():
    for n in ("louvain_csr", "modularity_csr", "Community", "make_leiden_clusters", "calc_modularity", "save_clusters_as_json",
              "save_clusters_as_csv"):
        assert n in nabo_amd.__all__ and callable(getattr(nabo_amd, n))
    assert callable(nabo_amd.RefGraph.make_leiden_clusters) and callable(nabo_amd.RefGraph.calc_modularity)
    src = open(os.path.join(REPO, "include", "nabo_community.h")).read()
    assert '#include "nabo_knn.h"' in src and "nabo_community.h" not in open(os.path.join(REPO, "include", "nabo_knn.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert sorted(set(re.findall(r"\b(nabo_[a-z0-9_]+)\s*\(", src))) == sorted(_lib.COMMUNITY_SYMBOLS)
    others = (_lib.SYMBOLS + _lib.GRAPH_SYMBOLS + _lib.CLUSTER_SYMBOLS + _lib.DE_SYMBOLS + _lib.PCA_SYMBOLS + _lib.PCA_FIT_SYMBOLS
              + _lib.QC_SYMBOLS + _lib.LAYOUT_SYMBOLS + _lib.UMAP_SYMBOLS)
    assert not set(_lib.COMMUNITY_SYMBOLS) & set(others)
    L = _lib.lib()
    for n in _lib.COMMUNITY_SYMBOLS:
        assert hasattr(L, n), n
    group, thr, cap = _community.geometry()
    assert group in (1, 2, 4, 8, 16, 32, 64) and group <= thr < cap
    hip = open(os.path.join(REPO, "nabo_amd", "csrc", "community.hip")).read()
    assert "CM_GROUP = %d;" % group in hip and "CM_LONG = %d;" % thr in hip and cap == 1 << int(re.search(r"CM_CAP_BITS = (\d+);", hip).group(1))


def test_header_is_plain_c_and_links(tmp_path):
    _lib.lib()
    exe = os.path.join(str(tmp_path), "community_check")
    cmd = ["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(REPO, "include"),
           os.path.join(REPO, "tests", "abi_c", "community_check.c"), "-L" + os.path.join(REPO, "nabo_amd"), "-lnabo_knn",
           "-Wl,-rpath," + os.path.join(REPO, "nabo_amd"), "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0 and "%d entry points" % len(_lib.COMMUNITY_SYMBOLS) in r.stdout, r.stdout


GOOD = dict(ptr=[0, 1, 2, 3], nbr=[1, 2, 0], w=[0.5, 0.25, 1.0])


@pytest.mark.parametrize("change", [
    {"ptr": [0, 1, 2]},                                      # does not end at len(nbr)
    {"ptr": [1, 1, 2, 3]},
    {"ptr": [0, 2, 1, 3]},                                   # not monotone
    {"ptr": [0]},                                            # no node
    {"nbr": [1, 2, 3]},                                      # no such node
    {"nbr": [1, 2, -1]},
    {"w": [0.5, 0.25]},                                      # another length than nbr
    {"w": [0.5, np.nan, 1.0]},
    {"w": [0.5, -0.25, 1.0]},
    {"w": [0.5, 0.25, 1e6]},                                 # quantises above 2^31
    {"resolution": -1.0},
    {"resolution": np.inf},
    {"resolution": "high"},
    {"weight_scale": 0},
    {"weight_scale": np.nan},
    {"seed": -1},
    {"seed": 1.5},
    {"max_sweeps": 0},
    {"max_levels": 0},
    {"max_levels": 2.0},
])
def test_bad_arguments_raise_before_any_device(change):
    with pytest.raises(ValueError) as e:
        nabo_amd.louvain_csr(**dict(GOOD, **change))
    assert str(e.value).startswith("ERROR: ")


@pytest.mark.parametrize("labels", [[1, 2], [1, 2, 3, 4], [1.5, 2.0, 1.0], [[1, 2, 3]], [1, 2, 2 ** 31], ["a", "b", "c"]])
def test_bad_labels_raise_before_any_device(labels):
    with pytest.raises(ValueError) as e:
        nabo_amd.modularity_csr(labels=labels, **GOOD)
    assert str(e.value).startswith("ERROR: ")


def test_no_device_is_a_loud_failure():
    if nabo_amd.device_count() > 0:
        pytest.skip("a GPU is visible here; the no-device path is covered on the CPU box")
    with pytest.raises(nabo_amd.NaboError) as e:
        nabo_amd.louvain_csr(**GOOD)
    assert "no HIP device" in str(e.value)


def test_hundredths_quantise_exactly():
    for fn in (_community.quantise, cr.quantise):
        q = fn([round(i / 100, 2) for i in range(101)] + [i / 100 for i in range(101)])
        assert q.dtype == np.int64 and q.tolist() == [100 * i for i in range(101)] * 2
    # Nabo's weights: round(s / (2 (k - 1) - s), 2) for every k and every count of shared neighbours, self included
    for k in range(3, 57):
        w = [round(s / (2 * (k - 1) - s), 2) for s in range(1, k + 1)]
        assert _community.quantise(w).tolist() == [int(round(x * 100)) * 100 for x in w]
    assert _community.quantise([0.00004, 0.00006]).tolist() == [0, 1]
    assert _community.quantise([0.25, 0.75, 1.25], 2).tolist() == [0, 2, 2]                       # rint: halves to even


def test_gate_follows_its_formula():
    mix = cr.mix_int
    for seed, level, s, n in ((4466, 0, 0, 100), (0, 3, 17, 5), (2 ** 64 - 1, 31, 127, 64)):
        want = [mix(mix(mix(seed + cr.GOLD * (level + 1)) + cr.GOLD * (s + 1)) + cr.GOLD * (i + 1)) >> 63 for i in range(n)]
        assert cr.active(seed, level, s, n).tolist() == [bool(x) for x in want]
    on = cr.active(4466, 0, 0, 4000).mean()
    assert 0.45 < on < 0.55


def check_invariants(ptr, nbr, w, labels, info, gamma, split):
    lv0, two_m = cr.level0(ptr, nbr, w)
    n = lv0.n
    assert labels.dtype == np.int32 and labels.shape == (n,)
    # labels 1 .. C by descending size, ties by smallest member
    C = info["n_clusters"]
    assert sorted(set(labels.tolist())) == list(range(1, C + 1))
    cnt = np.bincount(labels, minlength=C + 1)[1:]
    first = [int(np.flatnonzero(labels == c)[0]) for c in range(1, C + 1)]
    assert all((cnt[c] > cnt[c + 1]) or (cnt[c] == cnt[c + 1] and first[c] < first[c + 1]) for c in range(C - 1))
    # Q recomputed from the labels is the reported Q, and no worse than the singletons'
    assert cr.label_q(lv0, two_m, labels, gamma) == info["q"]
    assert info["q"] >= cr.level_q(lv0, two_m, gamma)
    assert sum(lv0.k.tolist()) == two_m == info["two_m"]
    if split:                                               # every community is connected
        assert np.array_equal(cr.finish(lv0, labels, True)[0], labels)
    for a, b in zip(info["history"], info["history"][1:]):
        assert a[1] == b[0]
    assert info["history"][0][0] == n


def test_yardstick_on_graphs_whose_answer_is_known():
    res = {name: cr.louvain(*g) for name, g in TINY.items()}
    for name, (labels, info) in res.items():
        check_invariants(*TINY[name], labels, info, 1.0, True)
    labels, info = res["two_k4_bridge"]
    assert labels.tolist() == [1, 1, 1, 1, 2, 2, 2, 2] and info["q"] == 0.42307692307692313
    labels, info = res["ring12"]                             # ties everywhere: the lowest id wins, the gate breaks the symmetry
    assert info["n_clusters"] == 4 and info["q"] == 0.40277777777777773
    assert res["k2"][1]["n_clusters"] == 1 and res["star9"][1]["n_clusters"] == 1
    assert res["k55"][1]["q"] == 0.0
    labels, info = res["loops_and_isolated"]                 # nobody has a neighbour: singletons, Q from the loops alone
    assert info["n_clusters"] == 6 and info["history"] == [(6, 6, 1, 0, info["q"])]
    assert info["q"] == 17500 / 35000 - (20000 ** 2 + 10000 ** 2 + 5000 ** 2) / 35000 ** 2
    # without the split the same partitions: these graphs' communities are connected already
    for name in ("two_k4_bridge", "ring12"):
        l2, i2 = cr.louvain(*TINY[name], split=False)
        assert np.array_equal(l2, res[name][0]) and i2["q"] == res[name][1]["q"]


@pytest.mark.parametrize("name", cr.CAPACITY_GRAPHS)
def test_capacity_graphs_meet_the_paths_they_were_made_for(name):
    """what tests/test_community_gpu.py relies on: 20 rows beyond the sweep's table in sweep 0 of many_over_capacity and
    the same rows at 1862 distinct communities in sweep 1, rows one under, at and one over the table, and rows longer
    than the long path's workgroup that fit -- from the yardstick alone"""
    _, long_threshold, cap = _community.geometry()
    hip = open(os.path.join(REPO, "nabo_amd", "csrc", "community.hip")).read()
    threads, blocks = (int(re.search(r"%s = (\d+);" % c, hip).group(1)) for c in ("CM_THREADS", "CM_HUGE_BLOCKS"))
    assert 20 > 2 * blocks                                   # every workgroup of the huge path takes more than one row
    ptr, nbr, w = cr.capacity_graphs(cap)[name]
    lv, two_m = cr.level0(ptr, nbr, w)
    cr.check_capacity_graph(name, lv, two_m, long_threshold, cap, 4466, workgroup=threads)


def test_split_takes_a_disconnected_community_apart():
    ptr, nbr, w = cr.csr_of_edges(9, cr.clique(0, 4) + cr.clique(4, 4))     # two cliques and an isolated node
    lv0, two_m = cr.level0(ptr, nbr, w)
    one = np.zeros(9, dtype=np.int64)
    kept, c1 = cr.finish(lv0, one, False)
    cut, c3 = cr.finish(lv0, one, True)
    assert c1 == 1 and kept.tolist() == [1] * 9
    assert c3 == 3 and cut.tolist() == [1] * 4 + [2] * 4 + [3]
    assert cr.label_q(lv0, two_m, cut, 1.0) > cr.label_q(lv0, two_m, kept, 1.0)
    assert cr.components(lv0, one).tolist() == [0] * 4 + [4] * 4 + [8]


def test_duplicates_self_loops_and_vanishing_weights():
    # (0, 1) listed three times, from both ends: the listing LAST IN THE ARRAYS wins, which is row 1's; (2, 3) quantises
    # to 0 and goes, its nodes stay
    ptr, nbr, w = cr.csr_of_edges(5, [(0, 1, 0.5), (1, 0, 0.25), (2, 3, 0.00004), (0, 1, 0.07), (4, 4, 0.3), (1, 4, 1.0)])
    assert nbr.tolist() == [1, 1, 0, 4, 3, 4] and w[:3].tolist() == [0.5, 0.07, 0.25]
    lv0, two_m = cr.level0(ptr, nbr, w)
    assert lv0.arc_set() == {(0, 1, 2500), (1, 0, 2500), (1, 4, 10000), (4, 1, 10000)}
    assert lv0.k.tolist() == [2500, 12500, 0, 0, 16000] and lv0.inn.tolist() == [0, 0, 0, 0, 3000] and two_m == 31000


def test_aggregation_keeps_the_weight():
    ptr, nbr, w = TINY["ring12"]
    lv0, two_m = cr.level0(ptr, nbr, w)
    comm = np.array([0, 0, 0, 5, 5, 5, 5, 7, 7, 11, 11, 0])
    nx, lab = cr.aggregate(lv0, comm)
    assert nx.n == 4 and lab.tolist() == [0, 0, 0, 1, 1, 1, 1, 2, 2, 3, 3, 0]
    assert nx.k.tolist() == [80000, 80000, 40000, 40000] and nx.inn.tolist() == [60000, 60000, 20000, 20000]
    assert nx.arc_set() == {(0, 1, 10000), (1, 0, 10000), (1, 2, 10000), (2, 1, 10000), (2, 3, 10000), (3, 2, 10000), (3, 0, 10000),
                            (0, 3, 10000)}
    assert int(nx.k.sum()) == two_m


@pytest.mark.parametrize("at", [0, 1, 2])
def test_yardstick_quality_against_networkx(gold, at):
    """networkx's louvain_communities ran on this graph for seeds 0-4 when the golden file was written; the yardstick
    may fall short of its worst run by no more than its own seed-to-seed spread"""
    gamma = float(gold["gammas"][at])
    labels, info = cr.louvain(gold["ptr"], gold["nbr"], gold["w"], resolution=gamma)
    rec = gold["nx_q"][at]
    print("resolution %g: yardstick Q = %.5f, networkx %s: %.5f .. %.5f" % (gamma, info["q"], str(gold["networkx_version"]), rec.min(), rec.max()))
    assert info["q"] >= rec.min() - (rec.max() - rec.min())
    assert info["q"] == float(gold["ref_q"][at]) and np.array_equal(labels, gold["ref_labels"][at]), \
        "the yardstick changed: run tools/gen_golden_community.py"
    check_invariants(gold["ptr"], gold["nbr"], gold["w"], labels, info, gamma, True)
    qs = [h[4] for h in info["history"]]
    assert qs == sorted(qs) and 30 <= info["history"][0][2] < 128       # monotone over levels; level 0 stops by itself


def test_float_loops_stay_within_their_bound(gold):
    ptr, nbr, w = gold["ptr"], gold["nbr"], gold["w"]
    lv0, two_m = cr.level0(ptr, nbr, w)
    labels = gold["ref_labels"][1]
    loops, adds, max_edges = cr.reference_loops_q(ptr, nbr, w, labels)
    exact = cr.label_q(lv0, two_m, labels, 1.0)
    print("float loops %.17g, exact %.17g, apart by %.3g (recorded %.3g) after %d additions" % (loops, exact, abs(loops - exact),
                                                                                            float(gold["loops_diff"]), adds))
    assert abs(loops - exact) <= cr.loops_bound(adds, max_edges) < 1e-8


def test_cluster_dict_modularity_and_writers(tmp_path, monkeypatch):
    pd = pytest.importorskip("pandas")
    ref_nodes = ["c%d_WT" % i for i in (2, 0, 1)]
    pos = {"c0_WT": 0, "c1_WT": 1, "c2_WT": 2}
    seen = {}

    def louvain(ptr, nbr, w, resolution, seed, device):
        seen.update(resolution=resolution, seed=seed, device=device)
        return np.array([2, 1, 1], dtype=np.int32), {"q": 0.25}

    monkeypatch.setattr(_community, "louvain_csr", louvain)
    clusters, info = _community._leiden_of_graph(ref_nodes, pos, [0, 1, 2, 2], [1, 2], [1.0, 1.0], 0.8, 7, 0)
    assert clusters == {"c2_WT": "1", "c0_WT": "2", "c1_WT": "1"} and list(clusters) == ref_nodes
    assert seen == dict(resolution=0.8, seed=7, device=0) and info["q"] == 0.25
    with pytest.raises(AssertionError) as e:
        _community._modularity_of_graph(ref_nodes, pos, [0, 1, 2, 2], [1, 2], [1.0, 1.0], {"c0_WT": "1", "c1_WT": "1"}, 0)
    assert str(e.value) == "ERROR: Not all reference nodes have been assigned to a cluster. Cannot calculate modularity!"
    fn = os.path.join(str(tmp_path), "clusters.json")
    nabo_amd.save_clusters_as_json(clusters, fn)
    assert json.load(open(fn)) == clusters and open(fn).read() == json.dumps(clusters, indent=2)
    fn = os.path.join(str(tmp_path), "clusters.csv")
    nabo_amd.save_clusters_as_csv(clusters, fn)
    ref = os.path.join(str(tmp_path), "pandas.csv")
    pd.Series(clusters).to_csv(ref)
    assert open(fn).read() == open(ref).read()
    back = pd.read_csv(fn, index_col=0, header=0)
    assert {k: str(v) for k, v in back[back.columns[0]].to_dict().items()} == clusters
