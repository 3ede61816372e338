"""The greedy modularity agglomeration on the MI355X (include/nabo_agglom.h, nabo_amd._community) against the tests' numpy /
Python-int restatement (tests/_agglom_ref.py).  Every quantity is an exact integer or comes from one, so the device must
EQUAL the yardstick: partners, gains, pairs, merge records and labels by equality, Q by its bytes.  One pass first, then
a round, then the whole run and its cuts, so that the first step that differs names the kernel at fault."""
import struct

import numpy as np
import pytest

from nabo_amd import _community

import _agglom_ref as ar
import _community_ref as cr

pytestmark = pytest.mark.gpu

GROUP, LONG, CAP = _community.geometry()
TINY = cr.tiny_graphs()
LONG_ROWS = [255, 256, 257, 600]                             # AG_THREADS = 256 (nabo_amd/csrc/agglom.hip)


def bits(x):
    return struct.pack("<d", float(x))


def hubs_graph(lengths, pool=200, seed=3):
    """one hub per entry of `lengths` with exactly that many neighbours, drawn from a weighted ring of `pool` leaves"""
    rng = np.random.default_rng(seed)
    edges = [(i, (i + 1) % pool, round(float(rng.integers(1, 101)) / 100, 2)) for i in range(pool)]
    for h, L in enumerate(lengths):
        for j in rng.choice(pool, size=L, replace=False).tolist():
            edges.append((pool + h, j, round(float(rng.integers(1, 101)) / 100, 2)))
    return cr.csr_of_edges(pool + len(lengths), edges)


def graphs():
    g = dict(TINY)
    g["hubs_edges"] = hubs_graph([GROUP - 1, GROUP, GROUP + 1, LONG, LONG + 1])
    # 4 has no neighbour at all, 5 only a self-loop; 0 and 3 carry self-loops so heavy that every gain at them is negative
    g["heavy_loops"] = cr.csr_of_edges(8, cr.clique(0, 4, 0.5) + [(0, 0, 90.0), (3, 3, 75.5), (5, 5, 1.0), (6, 7, 0.25), (1, 6, 0.01)])
    g["unit_ring"] = cr.csr_of_edges(30, [(i, (i + 1) % 30, 1.0) for i in range(30)])
    g["unit_clique"] = cr.csr_of_edges(9, cr.clique(0, 9))
    g["star70"] = cr.csr_of_edges(71, [(0, i, 1.0) for i in range(1, 71)])
    # long rows around and beyond one round of the long path's workgroup (256 lanes, an arc each per round)
    g["hubs_long"] = hubs_graph(LONG_ROWS, pool=700)
    g["two_parts"] = cr.csr_of_edges(11, cr.clique(0, 5, 0.3) + cr.clique(5, 6, 0.7))
    g["one_node"] = cr.csr_of_edges(1, [])
    g["no_arcs"] = cr.csr_of_edges(5, [(1, 1, 1.0)])
    return g


GRAPHS = graphs()


@pytest.fixture(scope="module")
def gold(golden):
    d = golden("community")
    return d["ptr"], d["nbr"].astype(np.int64), d["w"]


@pytest.fixture(scope="module")
def gold_run(gold):
    """the yardstick's whole run on the golden graph with its levels, computed once"""
    levels = []
    res = ar.run(*gold, levels=levels)
    return res, levels


def same_pass(H, lv, two_m, free=None):
    partner, D = H.match_pass(free)
    rp, rD, _ = ar.match_pass(lv, two_m, free)
    bad = np.flatnonzero(partner != rp)
    assert bad.size == 0, "%d rows differ, the first is %d (device %d, yardstick %d)" % (bad.size, bad[0], partner[bad[0]], rp[bad[0]])
    assert partner.dtype == np.int32 and D == rD.tolist()
    return rp


@pytest.mark.parametrize("name", list(GRAPHS))
def test_one_pass_on_the_constructed_graphs(gpu_lib, name):
    ptr, nbr, w = GRAPHS[name]
    lv, two_m = cr.level0(ptr, nbr, w)
    rows = np.bincount(lv.src, minlength=lv.n) if len(lv.src) else np.zeros(lv.n, dtype=np.int64)
    if name == "hubs_edges":                                 # the group's and the long path's edges
        assert rows[-5:].tolist() == [GROUP - 1, GROUP, GROUP + 1, LONG, LONG + 1] == [15, 16, 17, 64, 65]
    if name == "star70":
        assert rows[0] == 70 > LONG
    if name == "hubs_long":                                  # one below, at, one above and beyond two rounds of 256 lanes
        assert rows[-4:].tolist() == LONG_ROWS and rows[:-4].max() <= LONG
    rng = np.random.default_rng(1)
    with _community.Community(ptr, nbr, w) as H:
        rp = same_pass(H, lv, two_m)
        if name == "heavy_loops":
            assert rows[4] == 0 and rows[5] == 0 and rp[[0, 3, 4, 5]].tolist() == [-1, -1, -1, -1] and rp[1] == 2
        for frac in (0.5, 0.9, 0.0):                        # given masks; nobody free at the end
            same_pass(H, lv, two_m, rng.random(lv.n) < frac)
        if lv.n > 1:                                        # everybody but one: the hub, or node 0
            free = np.ones(lv.n, dtype=bool)
            free[int(np.argmax(rows))] = False
            same_pass(H, lv, two_m, free)


def test_one_pass_on_the_golden_graph_and_a_coarse_level(gpu_lib, gold):
    lv, two_m = cr.level0(*gold)
    rng = np.random.default_rng(2)
    with _community.Community(*gold) as H:
        same_pass(H, lv, two_m)
        same_pass(H, lv, two_m, rng.random(lv.n) < 0.6)
        # a coarse level, reached as the clustering reaches it: a phase of Louvain, then set_comm + aggregate
        comm, _, moved = cr.phase(lv, 1.0, two_m, 4466, 0, max_sweeps=6)
        assert moved > 0
        H.set_comm(comm)
        H.aggregate()
        nx, _ = cr.aggregate(lv, comm)
        assert H.level_size()[:2] == (nx.n, len(nx.src)) and nx.n < lv.n
        rp = same_pass(H, nx, two_m)
        assert (rp >= 0).sum() > 10
        same_pass(H, nx, two_m, rng.random(nx.n) < 0.5)


def wide_graph(n_bulk=1 << 16, reach=16, gadgets=8, seed=7):
    """Quantised weights near 2^31 and 2m near 2^52, as a Level made with numpy (the graph is simple by construction) and
    as the CSR the device gets (weight_scale 1).  A ring lattice of n_bulk nodes, each joined to the next `reach`, carries
    the weight.  Every gadget is a node c with two neighbours only, d' < d, a_cd = A and a_cd' = A - 1, and a pendant at
    each of d and d' that sets k_d - k_d' = delta; two filler pairs tune 2m to k_c delta + 1 or 2, so that
    D(c, d) - D(c, d') = 2m - k_c (k_d - k_d') is 1 or 2 while both gains are near 2^83: d wins, by less than float64
    resolves."""
    rng = np.random.default_rng(seed)
    A = (1 << 31) - 5
    i = np.repeat(np.arange(n_bulk, dtype=np.int64), reach)
    j = (i + np.tile(np.arange(1, reach + 1, dtype=np.int64), n_bulk)) % n_bulk
    q = (1 << 31) - rng.integers(0, 1 << 12, size=i.size).astype(np.int64)
    kc = 2 * A - 1
    xs = rng.integers(1000, 1 << 20, size=gadgets).astype(np.int64)       # the pendant weights at d'
    R = 2 * int(q.sum()) + gadgets * 2 * (2 * A - 1) + 4 * int(xs.sum()) - 2 * gadgets
    delta = -(-R // (kc - 2 * gadgets))
    eps = 2 if delta % 2 == 0 else 1
    T = ((kc - 2 * gadgets) * delta + eps - R) // 2
    assert 0 <= T < 1 << 32 and delta < 1 << 30
    ei, ej, eq = [i], [j], [q]
    n = n_bulk
    cs = []
    for g in range(gadgets):                                 # nodes: d', d, c, the pendant of d', the pendant of d
        dp, d, c, pp, pd = n, n + 1, n + 2, n + 3, n + 4
        ei.append(np.array([c, c, dp, d]))
        ej.append(np.array([d, dp, pp, pd]))
        eq.append(np.array([A, A - 1, xs[g], xs[g] + delta - 1]))
        cs.append(c)
        n += 5
    for t in (T // 2, T - T // 2):                           # the filler pairs
        if t:
            ei.append(np.array([n]))
            ej.append(np.array([n + 1]))
            eq.append(np.array([t]))
        n += 2
    ei, ej, eq = (np.concatenate(v).astype(np.int64) for v in (ei, ej, eq))
    src, dst, a = np.concatenate([ei, ej]), np.concatenate([ej, ei]), np.concatenate([eq, eq])
    o = np.lexsort((dst, src))
    k = np.zeros(n, dtype=np.int64)
    np.add.at(k, src, a)
    lv = cr.Level(n, src[o], dst[o], a[o], k, np.zeros(n, dtype=np.int64))
    two_m = int(k.sum())
    assert two_m == kc * delta + eps
    order = np.argsort(ei, kind="stable")
    ptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(ei, minlength=n), out=ptr[1:])
    return lv, two_m, (ptr, ej[order], eq[order].astype(np.float64)), np.array(cs)


def picks_of(lv, score):
    """per row the neighbour of largest score > 0, the first pair by ids on ties: the pass with another arithmetic"""
    ok = score > 0
    src, dst, s = lv.src[ok], lv.dst[ok], score[ok]
    o = np.lexsort((np.maximum(src, dst), np.minimum(src, dst), -s, src))
    first = o[np.flatnonzero(np.r_[True, src[o][1:] != src[o][:-1]])]
    out = np.full(lv.n, -1, dtype=np.int64)
    out[src[first]] = dst[first]
    return out


def test_the_gain_needs_all_128_bits(gpu_lib):
    lv, two_m, (ptr, nbr, w), cs = wide_graph()
    assert 2.0 ** 51.9 < two_m < 2.0 ** 52.1 and lv.a.max() <= 1 << 31 and lv.a.max() > (1 << 31) - (1 << 13)
    exact, D, _ = ar.match_pass(lv, two_m)
    assert max(D.tolist()) > 1 << 82
    # in float64, every operation rounded once
    f = picks_of(lv, lv.a.astype(np.float64) * np.float64(two_m) - lv.k[lv.src].astype(np.float64) * lv.k[lv.dst].astype(np.float64))
    # in wrapping 64-bit integers
    with np.errstate(over="ignore"):
        u = lv.a.astype(np.uint64) * np.uint64(two_m) - lv.k[lv.src].astype(np.uint64) * lv.k[lv.dst].astype(np.uint64)
    wr = picks_of(lv, u.view(np.int64))
    n_f, n_w = int((f != exact).sum()), int((wr != exact).sum())
    print("rows whose pick changes: %d in float64 (%d of them gadgets), %d in wrapping 64-bit" % (n_f, int((f[cs] != exact[cs]).sum()), n_w))
    assert (f[cs] != exact[cs]).any() and n_w > 0
    assert (exact[cs] == cs - 1).all()                       # d, by a gain that is 1 or 2 larger
    with _community.Community(ptr, nbr, w, weight_scale=1) as H:
        d = H.get_level()
        assert H.level_size() == (lv.n, len(lv.src), two_m) and np.array_equal(d["nbr"], lv.dst) and np.array_equal(d["a"], lv.a)
        assert np.array_equal(d["k"], lv.k)
        partner, Dd = H.match_pass()
    assert np.array_equal(partner, exact) and Dd == D.tolist()


def same_round(H, lv, two_m, pairs, passes):
    got, p = H.match()
    assert p == passes and got.dtype == np.int32
    assert got.tolist() == [[c, d] for c, d, _, _ in pairs]
    comm = ar.comm_of(lv.n, pairs)
    assert np.array_equal(H.get_comm(), comm)
    H.aggregate()
    nx, _ = cr.aggregate(lv, comm)
    d = H.get_level()
    assert H.level_size() == (nx.n, len(nx.src), two_m)
    assert np.array_equal(d["nbr"], nx.dst) and np.array_equal(d["a"], nx.a) and np.array_equal(d["k"], nx.k) and np.array_equal(d["in"], nx.inn)
    assert np.array_equal(d["ptr"], nx.csr()[0])
    return nx


def test_round_by_round_on_the_blob_graph(gpu_lib, gold, gold_run):
    """match + aggregate against the yardstick: the pairs in order, then the level arrays (the golden graph is
    blob_snn_graph(3000))"""
    res, levels = gold_run
    assert len(levels) == res["rounds"] == 16 and sum(p for _, _, p in levels) == res["passes"]
    with _community.Community(*gold) as H:
        for lv, pairs, passes in levels:
            nx = same_round(H, lv, res["two_m"], pairs, passes)
        assert nx.n == res["n_end"] and len(nx.src) == 0
        got, p = H.match()                                   # no arc is left: no pair, one pass
        assert got.shape == (0, 2) and p == 1


@pytest.mark.parametrize("name", ["unit_ring", "unit_clique", "star70", "two_k4_bridge", "k55", "heavy_loops", "hubs_edges", "hubs_long"])
def test_rounds_on_the_constructed_graphs(gpu_lib, name):
    ptr, nbr, w = GRAPHS[name]
    levels = []
    res = ar.run(ptr, nbr, w, levels=levels)
    if name in ("unit_ring", "unit_clique"):                 # equal weights: one pair a pass, the ids decide
        assert levels[0][2] > 2 and [t[1] for t in ar.match(levels[0][0], res["two_m"])[2][:-1]] == [1] * (levels[0][2] - 1)
    if name == "star70":                                     # every pair holds the hub: one merge a round, through the long path
        assert res["rounds"] == 70 and all(len(p) == 1 for _, p, _ in levels)
    if name == "heavy_loops":                                # the run's last rounds have no positive gain left
        assert any(p[0][2] <= 0 for _, p, _ in levels)
    with _community.Community(ptr, nbr, w) as H:
        for lv, pairs, passes in levels[:12]:
            same_round(H, lv, res["two_m"], pairs, passes)


def same_dendrogram(info, res):
    assert info["merges"].dtype == np.int64 and info["merges"].tobytes() == res["merges"].tobytes()
    assert info["q_path"].tobytes() == res["q_path"].tobytes()
    assert (info["rounds"], info["passes"], info["peak"], info["n_end"]) == (res["rounds"], res["passes"], res["peak"], res["n_end"])


def test_whole_run_on_the_golden_graph(gpu_lib, gold, gold_run, golden):
    res, _ = gold_run
    n0 = res["lv0"].n
    with _community.Community(*gold) as H:
        info = H.agglomerate()
        same_dendrogram(info, res)
        rec, q_path = H.dendrogram()
        assert rec.tobytes() == res["merges"].tobytes() and q_path.tobytes() == res["q_path"].tobytes()
        assert info["ms"]["run"] > 0 and info["ms"]["passes"] > 0
        cuts = {}
        for c in (res["n_end"], 8, 40, n0, 0):
            labels, C, q = H.cut(c)
            rl, rC, rq = ar.cut(res, c)
            assert labels.dtype == np.int32 and np.array_equal(labels, rl) and C == rC == len(set(labels.tolist()))
            assert bits(q) == bits(rq) == bits(H.modularity(labels, 1.0))
            cuts[c] = labels.tobytes(), q
        assert n0 - res["peak"] == 8 and cuts[0] == cuts[8]
        assert res["n_end"] == 7
        for bad in (1, 5, res["n_end"] - 1, n0 + 1):         # 1 and 5 lie below the 7 components of this graph
            with pytest.raises(ValueError):
                H.cut(bad)
        again = H.agglomerate()                              # two runs, identical bytes
        same_dendrogram(again, res)
        assert H.cut(40)[0].tobytes() == cuts[40][0]
    labels, info = gpu_lib.agglomerate_csr(*gold)
    assert labels.tobytes() == cuts[0][0] and info["n_clusters"] == 8 and bits(info["q"]) == bits(cuts[0][1])
    assert info["merges"].tobytes() == res["merges"].tobytes()
    labels, info = gpu_lib.agglomerate_csr(*gold, n_clusters=40)
    assert labels.tobytes() == cuts[40][0] and info["n_clusters"] == 40
    g = golden("agglom")
    assert np.array_equal(g["merges"], res["merges"]) and int(g["peak"]) == res["peak"]


def test_whole_run_on_a_connected_graph_down_to_one(gpu_lib):
    """the cuts at 1, 5, 8, 40, n0 and the peak on a graph that is connected, so that every one of them exists"""
    ptr, nbr, w = hubs_graph([GROUP + 1, LONG + 1, 3], pool=300, seed=5)
    res = ar.run(ptr, nbr, w)
    n0 = res["lv0"].n
    assert res["n_end"] == 1 and len(res["merges"]) == n0 - 1
    with _community.Community(ptr, nbr, w) as H:
        same_dendrogram(H.agglomerate(), res)
        for c in (1, 5, 8, 40, n0, 0):
            labels, C, q = H.cut(c)
            rl, rC, rq = ar.cut(res, c)
            assert np.array_equal(labels, rl) and C == rC == (c if c else n0 - res["peak"])
            assert bits(q) == bits(rq) == bits(H.modularity(labels, 1.0))
        # connected clusters by construction: the component split changes nothing
        assert np.array_equal(H.split(H.cut(8)[0], split=True)[0], H.cut(8)[0])


@pytest.mark.parametrize("name", list(GRAPHS))
def test_whole_run_on_the_constructed_graphs(gpu_lib, name):
    ptr, nbr, w = GRAPHS[name]
    res = ar.run(ptr, nbr, w)
    with _community.Community(ptr, nbr, w) as H:
        same_dendrogram(H.agglomerate(), res)
        for c in sorted({res["n_end"], res["lv0"].n, 0}):
            labels, C, q = H.cut(c)
            rl, rC, rq = ar.cut(res, c)
            assert np.array_equal(labels, rl) and C == rC and bits(q) == bits(rq) == bits(H.modularity(labels, 1.0))


def test_ends_and_errors(gpu_lib):
    ptr, nbr, w = GRAPHS["two_parts"]                        # two components: the run ends at 2 clusters
    with _community.Community(ptr, nbr, w) as H:
        with pytest.raises(ValueError):
            H.cut(2)                                         # no run yet
        info = H.agglomerate()
        assert info["n_end"] == 2 and len(info["merges"]) == 9
        assert H.cut(2)[0].tolist() == [2] * 5 + [1] * 6
        for bad in (1, 12):
            with pytest.raises(ValueError) as e:
                H.cut(bad)
            assert str(e.value).startswith("ERROR: ")
        for bad in (0, 12, 1.5):
            with pytest.raises(ValueError):
                H.agglomerate(bad)
    # n_min in the middle of a round: the prefix of the round
    ptr, nbr, w = hubs_graph([GROUP + 1, LONG + 1], pool=120, seed=8)
    full = ar.run(ptr, nbr, w)
    first = int((full["merges"][:, 2] == 0).sum())
    assert first > 4
    n_min = full["lv0"].n - (first - 3)
    res = ar.run(ptr, nbr, w, n_min=n_min)
    assert res["rounds"] == 1 and res["n_end"] == n_min and np.array_equal(res["merges"], full["merges"][:first - 3])
    with _community.Community(ptr, nbr, w) as H:
        same_dendrogram(H.agglomerate(n_min), res)
        assert H.level_size()[0] == n_min
        assert np.array_equal(H.cut(n_min)[0], ar.cut(full, n_min)[0])
        with pytest.raises(ValueError):
            H.cut(n_min - 1)
        same_dendrogram(H.agglomerate(full["lv0"].n), ar.run(ptr, nbr, w, n_min=full["lv0"].n))      # nothing to do
        assert H.cut(0)[1] == full["lv0"].n
    with pytest.raises(ValueError):
        gpu_lib.agglomerate_csr(*GRAPHS["two_parts"], n_clusters=1)


def test_rows_in_file_order(gpu_lib):
    """what make_clusters does with the graph it reads, without an HDF5 file: the dict is keyed in the rows' order, values
    are str, and another n_clusters on the same handle runs only the cut"""
    ptr, nbr, w = hubs_graph([GROUP + 1, LONG + 1, 3], pool=300, seed=5)
    n = len(ptr) - 1
    names = ["c%03d_WT" % i for i in range(n)]
    pos = {x: i for i, x in enumerate(names)}
    rows = [names[i] for i in np.random.default_rng(2).permutation(n)]
    res = ar.run(ptr, nbr, w)
    with _community.Community(ptr, nbr, w) as H:
        H.agglomerate()
        for c in (6, 17):
            clusters = _community._clusters_of_graph(rows, pos, H, c)
            labels = ar.cut(res, c)[0]
            assert list(clusters) == rows and clusters == {x: str(int(labels[pos[x]])) for x in rows}
            assert len(set(clusters.values())) == c
        with pytest.raises(ValueError):
            _community._clusters_of_graph(rows, pos, H, n + 1)


@pytest.mark.parametrize("graph_layout", ["per_node", "columnar"])
def test_make_clusters_on_a_mapping_file(gpu_lib, golden, tmp_path, graph_layout):
    pytest.importorskip("h5py")
    from _graph_case import build_file
    fn, _, _ = build_file(str(tmp_path), golden("mapping_small"), graph_layout=graph_layout, tag=graph_layout)
    ref_nodes, pos, n_ref, ptr, nbr, w = _community._ref_graph_csr(fn, "WT")
    res = ar.run(ptr, nbr, w)
    n_clusters = max(res["n_end"], 4)
    clusters = gpu_lib.make_clusters(fn, "WT", n_clusters)
    labels = ar.cut(res, n_clusters)[0]
    assert list(clusters) == ref_nodes and clusters == {x: str(int(labels[pos[x]])) for x in ref_nodes}
    assert len(set(clusters.values())) == n_clusters
    with gpu_lib.RefGraph(fn, "WT") as g:
        assert g.make_clusters(n_clusters) == clusters and g.clusters == clusters
        more = g.make_clusters(n_clusters + 3)               # the dendrogram is kept: only the cut runs
        assert len(set(more.values())) == n_clusters + 3 and g.clusters == more
        assert bits(g.calc_modularity()) == bits(ar.cut(res, n_clusters + 3)[2])
        with pytest.raises(ValueError):
            g.make_clusters(len(ptr))
    with pytest.raises(ValueError):
        gpu_lib.make_clusters(fn, "WT", len(ptr))
    # the dict goes straight into the consumers
    out = gpu_lib.classify_target(fn, "WT", "ME", cluster_dict=clusters)
    assert len(out) > 0 and set(out.values()) <= set(clusters.values()) | {"NA"}
