"""The clustering on the MI355X (nabo_community_*, nabo_amd._community) against the tests' numpy restatement of
include/nabo_community.h (tests/_community_ref.py).  Every sum is an integer one, so the device must EQUAL the yardstick:
integers and labels by array_equal, Q by its bytes.  A run is held to the yardstick ONE STEP AT A TIME -- a sweep from the
yardstick's comm, an aggregation from the yardstick's phase -- so that the first step that differs names the kernel at
fault; whole runs, determinism and the modularity of given labels come after."""
import struct

import numpy as np
import pytest

from nabo_amd import _community

import _community_ref as cr

pytestmark = pytest.mark.gpu

GROUP, LONG, CAP = _community.geometry()
SEED = 4466
N_SWEEPS = 8
TINY = cr.tiny_graphs()


def bits(x):
    return struct.pack("<d", float(x))


hubs_graph = cr.hubs_graph


def odds_graph():
    """isolated nodes, nodes with only a self-loop, duplicate arcs with different weights, arcs that quantise to 0, two
    singletons facing each other, beside a small weighted clique"""
    edges = cr.clique(0, 5, 0.37) + [(5, 5, 0.5), (6, 6, 1.22),           # 5, 6: only a self-loop; 7, 8: isolated
                                     (9, 10, 1.0),                        # two singletons facing each other
                                     (11, 12, 0.5), (12, 11, 0.25), (11, 12, 0.07), (12, 13, 0.3), (13, 13, 0.1),
                                     (14, 15, 0.00004), (15, 0, 0.00003), (14, 1, 0.2), (3, 3, 0.9)]
    return cr.csr_of_edges(16, edges)


def dense_planted_graph(n=240, groups=4, deg=3 * LONG, seed=9):
    """every row long: each node draws `deg` partners, three in four from its own planted group"""
    rng = np.random.default_rng(seed)
    grp = np.arange(n) % groups
    edges = []
    for i in range(n):
        own, rest = np.flatnonzero((grp == grp[i]) & (np.arange(n) != i)), np.flatnonzero(grp != grp[i])
        for j in np.concatenate([rng.choice(own, size=min(len(own), deg * 3 // 4), replace=False),
                                 rng.choice(rest, size=deg // 4, replace=False)]).tolist():
            edges.append((i, j, round(float(rng.integers(1, 123)) / 100, 2)))
    return cr.csr_of_edges(n, edges)


def graphs():
    g = dict(TINY)
    g["dense_planted"] = dense_planted_graph()
    g["hubs_group"] = hubs_graph([GROUP - 1, GROUP, GROUP + 1])
    g["hubs_threshold"] = hubs_graph([LONG - 1, LONG, LONG + 1, 3 * LONG])
    g["star_over_capacity"] = cr.csr_of_edges(CAP + 2, [(0, i, round((1 + i % 7) / 100, 2)) for i in range(1, CAP + 2)])
    g.update(cr.capacity_graphs(CAP))                          # many overflow rows, the table's edge, long rows that fit
    g["odds"] = odds_graph()
    g["unit_clique"] = cr.csr_of_edges(7, cr.clique(0, 7))
    g["one_node"] = cr.csr_of_edges(1, [])
    g["one_node_loop"] = cr.csr_of_edges(1, [(0, 0, 1.0)])
    g["two_nodes_apart"] = cr.csr_of_edges(2, [])
    g["no_arcs"] = cr.csr_of_edges(40, [])
    g["all_vanish"] = cr.csr_of_edges(4, [(0, 1, 0.00001), (2, 3, 0.00002)])
    return g


GRAPHS = graphs()


@pytest.fixture(scope="module")
def gold(golden):
    d = golden("community")
    return d["ptr"], d["nbr"].astype(np.int64), d["w"], d


@pytest.fixture(scope="module")
def gold_runs(gold):
    """the yardstick's whole runs on the golden graph, computed once"""
    cache = {}

    def run(gamma, split):
        if (gamma, split) not in cache:
            cache[(gamma, split)] = cr.louvain(gold[0], gold[1], gold[2], resolution=gamma, split=split)
        return cache[(gamma, split)]
    return run


def same_level(H, lv, two_m):
    d = H.get_level()
    n, A, m2 = H.level_size()
    assert (n, A, m2) == (lv.n, len(lv.src), two_m)
    src = np.repeat(np.arange(n), np.diff(d["ptr"]))
    assert d["ptr"][0] == 0 and d["ptr"][-1] == A
    assert set(zip(src.tolist(), d["nbr"].tolist(), d["a"].tolist())) == lv.arc_set() and len(set(zip(src.tolist(), d["nbr"].tolist()))) == A
    assert np.array_equal(d["k"], lv.k) and np.array_equal(d["in"], lv.inn)
    assert int(d["k"].sum()) == two_m
    for i in range(n):                                       # rows in ascending neighbour
        assert (np.diff(d["nbr"][d["ptr"][i]:d["ptr"][i + 1]]) > 0).all()


def step_through(ptr, nbr, w, gamma, levels=2):
    """sweeps 0 .. N_SWEEPS-1 of level 0 and of level 1, each from the yardstick's comm, and the aggregation between;
    returns what was exercised"""
    lv, two_m = cr.level0(ptr, nbr, w)
    seen = {"sweeps": 0, "moved": 0, "levels": 0, "emptied": False}
    with _community.Community(ptr, nbr, w, resolution=gamma, seed=SEED) as H:
        same_level(H, lv, two_m)
        for level in range(levels):
            trace = []
            comm, sweeps, moved = cr.phase(lv, gamma, two_m, SEED, level, trace=trace)
            for s, (before, after, mv, want) in enumerate(trace[:N_SWEEPS]):
                H.set_comm(before)
                got = H.sweep(level, s)
                assert got == (mv, want), "level %d sweep %d: (moved, want) = %r, the yardstick has %r" % (level, s, got, (mv, want))
                dev = H.get_comm()
                bad = np.flatnonzero(dev != after)
                assert bad.size == 0, "level %d sweep %d: %d nodes differ, the first is %d (device %d, yardstick %d)" % (
                    level, s, bad.size, bad[0], dev[bad[0]], after[bad[0]])
                seen["sweeps"] += 1
                seen["moved"] += mv
            if moved == 0:
                break
            H.set_comm(comm)
            H.aggregate()
            nx, _ = cr.aggregate(lv, comm)
            same_level(H, nx, two_m)
            assert np.array_equal(H.get_comm(), np.arange(nx.n))
            seen["emptied"] |= nx.n < lv.n and int(comm.max()) >= nx.n
            seen["levels"] += 1
            lv = nx
        H.rewind()
        assert H.level_size()[0] == len(ptr) - 1 and np.array_equal(H.get_comm(), np.arange(len(ptr) - 1))
    return seen


@pytest.mark.parametrize("gamma", [0.5, 1.0, 2.0])
def test_golden_graph_one_step_at_a_time(gpu_lib, gold, gamma):
    seen = step_through(gold[0], gold[1], gold[2], gamma)
    assert seen["sweeps"] == 2 * N_SWEEPS and seen["moved"] > 1000 and seen["levels"] == 2 and seen["emptied"]


@pytest.mark.parametrize("name", list(GRAPHS))
def test_constructed_graphs_one_step_at_a_time(gpu_lib, name):
    ptr, nbr, w = GRAPHS[name]
    lv, two_m = cr.level0(ptr, nbr, w)
    rows = np.bincount(lv.src, minlength=lv.n) if len(lv.src) else np.zeros(lv.n, dtype=np.int64)
    # the graphs meet the paths they were made for
    if name == "hubs_group":
        assert rows[-3:].tolist() == [GROUP - 1, GROUP, GROUP + 1]
    if name == "hubs_threshold":
        assert rows[-4:].tolist() == [LONG - 1, LONG, LONG + 1, 3 * LONG]
    if name == "star_over_capacity":
        assert rows[0] == CAP + 1 and rows[1:].max() == 1
    if name == "dense_planted":
        assert rows.min() > LONG
    if name in cr.CAPACITY_GRAPHS:
        cr.check_capacity_graph(name, lv, two_m, LONG, CAP, SEED)
        assert N_SWEEPS >= 2                                 # many_over_capacity: sweep 0 overflows, sweep 1 fits at 91 % load
    if name == "odds":
        assert rows[[5, 6, 7, 8]].tolist() == [0, 0, 0, 0] and lv.inn[[5, 6]].tolist() == [5000, 12200] and rows[15] == 0
        assert (11, 12, 2500) in lv.arc_set()
    seen = step_through(ptr, nbr, w, 1.0)
    if name in ("one_node", "one_node_loop", "two_nodes_apart", "no_arcs", "all_vanish", "loops_and_isolated"):
        assert seen["moved"] == 0 and seen["levels"] == 0
    else:
        assert seen["moved"] > 0 and seen["levels"] >= 1


def test_ties_go_to_the_lowest_id_and_singletons_do_not_swap(gpu_lib):
    # a unit clique from singletons: every score ties, so every node wants community 0 -- but 0 itself, which looks at
    # 1 .. 6, is held by the swap rule (best > own, both singletons)
    ptr, nbr, w = GRAPHS["unit_clique"]
    lv, two_m = cr.level0(ptr, nbr, w)
    with _community.Community(ptr, nbr, w, seed=SEED) as H:
        moved, want = H.sweep(0, 0)
        comm = H.get_comm()
    act = cr.active(SEED, 0, 0, 7)
    assert want == 6 and moved == int(act[1:].sum())
    assert comm.tolist() == [0] + [0 if a else i for i, a in enumerate(act.tolist()) if i > 0]
    # two singletons facing each other: only the higher one wants to move
    ptr, nbr, w = TINY["k2"]
    with _community.Community(ptr, nbr, w, seed=SEED) as H:
        sweeps = [H.sweep(0, s) + (H.get_comm().tolist(),) for s in range(4)]
    want = [w_ for _, w_, _ in sweeps]
    assert want[0] == 1 and sweeps[-1][2] in ([0, 0], [0, 1]) and all(c[0] == 0 for _, _, c in sweeps)


def same_run(got, ref):
    labels, info = got
    rl, ri = ref
    assert np.array_equal(labels, rl) and labels.dtype == np.int32
    assert info["n_clusters"] == ri["n_clusters"] and info["two_m"] == ri["two_m"]
    assert bits(info["q"]) == bits(ri["q"])
    assert [h[:4] for h in info["history"]] == [h[:4] for h in ri["history"]]
    assert [bits(h[4]) for h in info["history"]] == [bits(h[4]) for h in ri["history"]]


@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("gamma", [0.5, 1.0, 2.0])
def test_whole_run_on_the_golden_graph(gpu_lib, gold, gold_runs, gamma, split):
    got = gpu_lib.louvain_csr(gold[0], gold[1], gold[2], resolution=gamma, split=split)
    same_run(got, gold_runs(gamma, split))
    if split:
        at = gold[3]["gammas"].tolist().index(gamma)
        assert np.array_equal(got[0], gold[3]["ref_labels"][at]) and bits(got[1]["q"]) == bits(gold[3]["ref_q"][at])
    assert got[1]["ms"]["run"] > 0


@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("name", list(GRAPHS))
def test_whole_run_on_the_constructed_graphs(gpu_lib, name, split):
    ptr, nbr, w = GRAPHS[name]
    same_run(gpu_lib.louvain_csr(ptr, nbr, w, split=split), cr.louvain(ptr, nbr, w, split=split))


def test_run_options(gpu_lib, gold):
    """another seed, a cap on the sweeps and on the levels, another scale: each equal to the yardstick under the same"""
    ptr, nbr, w = GRAPHS["hubs_threshold"]
    for kw in (dict(seed=1), dict(max_sweeps=3), dict(max_levels=1), dict(weight_scale=100), dict(resolution=0.0),
               dict(seed=2 ** 64 - 1, max_sweeps=5, max_levels=2)):
        same_run(gpu_lib.louvain_csr(ptr, nbr, w, **kw), cr.louvain(ptr, nbr, w, **kw))


def test_split_takes_a_disconnected_community_apart(gpu_lib):
    ptr, nbr, w = cr.csr_of_edges(9, cr.clique(0, 4) + cr.clique(4, 4))     # two cliques far apart and an isolated node
    lv0, two_m = cr.level0(ptr, nbr, w)
    one = np.zeros(9, dtype=np.int32)
    with _community.Community(ptr, nbr, w, max_levels=1) as H:
        H.set_comm(one)                                     # forced into one community
        H.aggregate()
        d = H.get_level()
        assert H.level_size()[:2] == (1, 0) and d["k"].tolist() == [two_m] and d["in"].tolist() == [two_m]
        kept, c1 = H.split(one, split=False)
        cut, c3 = H.split(one, split=True)
        q1, q3 = H.modularity(kept), H.modularity(cut)
    assert c1 == 1 and kept.tolist() == [1] * 9
    assert c3 == 3 and cut.tolist() == [1] * 4 + [2] * 4 + [3]            # the split changed something
    assert np.array_equal(cut, cr.finish(lv0, one, True)[0]) and np.array_equal(kept, cr.finish(lv0, one, False)[0])
    assert bits(q1) == bits(cr.label_q(lv0, two_m, kept, 1.0)) and bits(q3) == bits(cr.label_q(lv0, two_m, cut, 1.0)) and q3 > q1


def test_split_of_arbitrary_parts_on_the_golden_graph(gpu_lib, gold):
    """parts that cut across the graph at random have many components each: long chains of labels for the pointer jumps"""
    lv0, two_m = cr.level0(gold[0], gold[1], gold[2])
    part = np.random.default_rng(5).integers(0, 3, size=lv0.n).astype(np.int32) * 7 - 3
    with _community.Community(gold[0], gold[1], gold[2]) as H:
        for split in (True, False):
            got, c = H.split(part, split=split)
            want, wc = cr.finish(lv0, part, split)
            assert c == wc and np.array_equal(got, want)
    assert wc == 3 and c == 3


def test_two_runs_are_bit_identical_and_equal_stepping_by_hand(gpu_lib, gold):
    ptr, nbr, w = gold[0], gold[1], gold[2]
    with _community.Community(ptr, nbr, w, resolution=1.0, seed=SEED) as H:
        a = H.run()
        b = H.run()
        assert a[0].tobytes() == b[0].tobytes() and bits(a[1]["q"]) == bits(b[1]["q"]) and a[1]["history"] == b[1]["history"]
        # by hand: sweep until a sweep reports want == 0, aggregate, go on; the composed map is the partition
        H.rewind()
        n = H.level_size()[0]
        part, history, best, best_q = np.arange(n), [], np.arange(n), H.modularity(np.arange(n))
        for level in range(32):
            n_level, moved = H.level_size()[0], 0
            for s in range(128):
                mv, want = H.sweep(level, s)
                moved += mv
                if want == 0:
                    break
            if moved == 0:
                history.append((n_level, n_level, s + 1, 0))
                break
            comm = H.get_comm()
            H.aggregate()
            part = (np.searchsorted(np.unique(comm), comm))[part]
            history.append((n_level, H.level_size()[0], s + 1, moved))
            q = H.modularity(part)
            if q > best_q:
                best, best_q = part, q
        labels, C = H.split(best.astype(np.int32), split=True)
        assert [h[:4] for h in a[1]["history"]] == history and C == a[1]["n_clusters"]
        assert labels.tobytes() == a[0].tobytes() and bits(H.modularity(labels)) == bits(a[1]["q"])
    c = gpu_lib.louvain_csr(ptr, nbr, w, resolution=1.0, seed=SEED)
    assert c[0].tobytes() == a[0].tobytes() and c[1]["history"] == a[1]["history"]


def test_modularity_of_given_labels(gpu_lib, gold):
    ptr, nbr, w, d = gold
    lv0, two_m = cr.level0(ptr, nbr, w)
    rng = np.random.default_rng(11)
    cases = [d["ref_labels"][1], np.arange(lv0.n), np.zeros(lv0.n, dtype=np.int64), rng.integers(-5, 40, size=lv0.n),
             rng.integers(-2 ** 31, 2 ** 31, size=lv0.n)]
    for labels in cases:
        for gamma in (1.0, 0.5, 2.0, 0.0):
            assert bits(gpu_lib.modularity_csr(ptr, nbr, w, labels, resolution=gamma)) == bits(cr.label_q(lv0, two_m, labels, gamma))
    # against the reference's float loops: within the bound its number of additions gives
    labels = d["ref_labels"][1]
    loops, adds, max_edges = cr.reference_loops_q(ptr, nbr, w, labels)
    q = gpu_lib.modularity_csr(ptr, nbr, w, labels)
    print("device %.17g, calc_modularity's float loops %.17g: apart by %.3g (recorded %.3g), bound %.3g after %d additions"
          % (q, loops, abs(q - loops), float(d["loops_diff"]), cr.loops_bound(adds, max_edges), adds))
    assert abs(q - loops) <= cr.loops_bound(adds, max_edges)
    # duplicates, self-loops and vanishing weights are read as the yardstick reads them
    ptr, nbr, w = GRAPHS["odds"]
    lv0, two_m = cr.level0(ptr, nbr, w)
    labels = np.arange(16) // 3
    assert bits(gpu_lib.modularity_csr(ptr, nbr, w, labels)) == bits(cr.label_q(lv0, two_m, labels, 1.0))
    assert gpu_lib.modularity_csr(*GRAPHS["all_vanish"], labels=[0, 0, 1, 1]) == 0.0


def test_rows_in_file_order(gpu_lib, gold):
    """what make_leiden_clusters and calc_modularity do with the graph they read, without an HDF5 file: the dict is keyed
    in the rows' order, values are str, and its modularity is the run's"""
    ptr, nbr, w = GRAPHS["hubs_threshold"]
    n = len(ptr) - 1
    names = ["c%03d_WT" % i for i in range(n)]
    pos = {x: i for i, x in enumerate(names)}
    rows = [names[i] for i in np.random.default_rng(2).permutation(n)]
    clusters, info = _community._leiden_of_graph(rows, pos, ptr, nbr, w, 1.0, SEED, 0)
    labels, ref = cr.louvain(ptr, nbr, w)
    assert list(clusters) == rows and clusters == {x: str(int(labels[pos[x]])) for x in rows} and bits(info["q"]) == bits(ref["q"])
    assert bits(_community._modularity_of_graph(rows, pos, ptr, nbr, w, clusters, 0)) == bits(info["q"])
    with pytest.raises(AssertionError):
        _community._modularity_of_graph(rows, pos, ptr, nbr, w, {x: clusters[x] for x in rows[1:]}, 0)


@pytest.mark.parametrize("graph_layout", ["per_node", "columnar"])
def test_make_leiden_clusters_on_a_mapping_file(gpu_lib, golden, tmp_path, graph_layout):
    pytest.importorskip("h5py")
    from _graph_case import build_file
    fn, _, _ = build_file(str(tmp_path), golden("mapping_small"), graph_layout=graph_layout, tag=graph_layout)
    ref_nodes, pos, n_ref, ptr, nbr, w = _community._ref_graph_csr(fn, "WT")
    clusters = gpu_lib.make_leiden_clusters(fn, "WT")
    labels, info = gpu_lib.louvain_csr(ptr, nbr, w)
    assert list(clusters) == ref_nodes and clusters == {x: str(int(labels[pos[x]])) for x in ref_nodes}
    assert len(set(clusters.values())) == info["n_clusters"] >= 2
    assert bits(gpu_lib.calc_modularity(fn, "WT", clusters)) == bits(info["q"])
    same_run((labels, info), cr.louvain(ptr, nbr, w))
    with gpu_lib.RefGraph(fn, "WT") as g:
        assert g.make_leiden_clusters() == clusters and g.clusters == clusters and bits(g.calc_modularity()) == bits(info["q"])
    with pytest.raises(AssertionError):
        gpu_lib.calc_modularity(fn, "WT", {x: clusters[x] for x in ref_nodes[1:]})
    # the dict goes straight into the consumers
    out = gpu_lib.classify_target(fn, "WT", "ME", cluster_dict=clusters)
    assert len(out) > 0 and set(out.values()) <= set(clusters.values()) | {"NA"}
    assert gpu_lib.classify_target(fn, "WT", "ME", clusters=clusters) is not None
    res = gpu_lib.get_de_groups(fn, "WT", "ME", 0.0, 1, clusters=clusters, from_clusters=["1"])
    assert res is None or set(res["de_group"].values()) <= {"Test", "Control", "Other"}
