"""numpy restatement of include/nabo_community.h, the yardstick of the community tests: the simple quantised graph, one
synchronous sweep, a phase, the aggregation, the modularity from exact integers (Python ints), the component split and
the final numbering.  Written from the header's definition with sorts and segmented sums; nothing here is shared with
the device code.  Every integer sum stays below 2^53 and is taken in int64."""
import numpy as np

M64 = (1 << 64) - 1
GOLD = 0x9E3779B97F4A7C15


def mix_int(z):
    z &= M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def mix_arr(z):
    z = z.astype(np.uint64)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def active(seed, level, sweep, n):
    """step 7: the gate of every node of a level's sweep"""
    h2 = mix_int(mix_int(seed + GOLD * (level + 1)) + GOLD * (sweep + 1))
    i = np.arange(1, n + 1, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = mix_arr(np.uint64(h2) + np.uint64(GOLD) * i)
    return (z >> np.uint64(63)) != 0


def quantise(w, weight_scale=10000):
    return np.rint(np.asarray(w, dtype=np.float64) * float(weight_scale)).astype(np.int64)


class Level:
    """n nodes; the off-diagonal arcs (src, dst, a), both directions, sorted by (src, dst); k and inn per node"""

    def __init__(self, n, src, dst, a, k, inn):
        self.n, self.src, self.dst, self.a, self.k, self.inn = int(n), src, dst, a, k, inn

    def csr(self):
        ptr = np.zeros(self.n + 1, dtype=np.int64)
        np.cumsum(np.bincount(self.src, minlength=self.n), out=ptr[1:])
        return ptr, self.dst, self.a

    def arc_set(self):
        return set(zip(self.src.tolist(), self.dst.tolist(), self.a.tolist()))


def level0(ptr, nbr, w, weight_scale=10000):
    """the simple quantised graph: a pair keeps its LAST weight, pairs of weight 0 are dropped, self-loops go to inn"""
    ptr, nbr, w = np.asarray(ptr, dtype=np.int64), np.asarray(nbr, dtype=np.int64), np.asarray(w, dtype=np.float64)
    n = len(ptr) - 1
    row = np.repeat(np.arange(n, dtype=np.int64), np.diff(ptr))
    lo, hi = np.minimum(row, nbr), np.maximum(row, nbr)
    last = {}
    for e in range(len(nbr)):                       # later entries overwrite: the last weight stays
        last[(int(lo[e]), int(hi[e]))] = float(w[e])
    pairs = sorted(last)
    q = quantise([last[p] for p in pairs], weight_scale) if pairs else np.zeros(0, dtype=np.int64)
    assert (q >= 0).all() and (q <= 2 ** 31).all()
    k, inn = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    src, dst, a = [], [], []
    for (i, j), x in zip(pairs, q.tolist()):
        if x == 0:
            continue
        if i == j:
            k[i] += 2 * x
            inn[i] = x
        else:
            k[i] += x
            k[j] += x
            src += [i, j]
            dst += [j, i]
            a += [x, x]
    src, dst, a = (np.array(v, dtype=np.int64) for v in (src, dst, a))
    o = np.lexsort((dst, src))
    lv = Level(n, src[o], dst[o], a[o], k, inn)
    assert int(k.sum()) < 2 ** 53
    return lv, int(k.sum())


def _segments(key):
    o = np.argsort(key, kind="stable")
    ks = key[o]
    starts = np.flatnonzero(np.r_[True, ks[1:] != ks[:-1]])
    return o, ks[starts], starts


def sweep(lv, comm, gamma, two_m, seed, level, s):
    """one synchronous sweep: (the new comm, moved, want)"""
    n = lv.n
    comm = np.asarray(comm, dtype=np.int64)
    if len(lv.src) == 0:
        return comm.copy(), 0, 0
    tot = np.zeros(n, dtype=np.int64)
    np.add.at(tot, comm, lv.k)
    size = np.bincount(comm, minlength=n)
    nb = np.flatnonzero(np.bincount(lv.src, minlength=n) > 0)          # the nodes with a neighbour j != i
    # candidates: every (i, community of a neighbour), plus (i, own community) with weight 0
    ci = np.concatenate([lv.src, nb])
    cc = np.concatenate([comm[lv.dst], comm[nb]])
    ca = np.concatenate([lv.a, np.zeros(len(nb), dtype=np.int64)])
    o, keys, starts = _segments(ci * n + cc)
    e = np.add.reduceat(ca[o], starts)
    ci, cc = keys // n, keys % n
    t = (float(gamma) * lv.k.astype(np.float64)) / np.float64(two_m)
    own = cc == comm[ci]
    T = tot[cc] - np.where(own, lv.k[ci], 0)
    prod = t[ci] * T.astype(np.float64)                                # rounded once
    score = e.astype(np.float64) - prod                                # rounded once
    o2 = np.lexsort((cc, -score, ci))                                  # per node: score descending, then community ascending
    first = o2[np.flatnonzero(np.r_[True, ci[o2][1:] != ci[o2][:-1]])]
    node, best, best_s = ci[first], cc[first], score[first]
    score_a = np.empty(n, dtype=np.float64)
    score_a[ci[own]] = score[own]
    a_of = comm[node]
    want = (best != a_of) & (best_s > score_a[node]) & ~((size[a_of] == 1) & (size[best] == 1) & (best > a_of))
    act = active(seed, level, s, n)[node]
    new = comm.copy()
    mv = want & act
    new[node[mv]] = best[mv]
    return new, int(mv.sum()), int(want.sum())


def phase(lv, gamma, two_m, seed, level, max_sweeps=128, comm=None, trace=None):
    """(comm, sweeps, moved); trace: a list that receives (comm before, comm after, moved, want) per sweep"""
    comm = np.arange(lv.n, dtype=np.int64) if comm is None else np.asarray(comm, dtype=np.int64)
    moved = sweeps = 0
    for s in range(max_sweeps):
        new, mv, want = sweep(lv, comm, gamma, two_m, seed, level, s)
        if trace is not None:
            trace.append((comm, new, mv, want))
        comm, moved, sweeps = new, moved + mv, s + 1
        if want == 0:
            break
    return comm, sweeps, moved


def aggregate(lv, comm):
    """(the coarse level, lab): lab[i] the new id of node i's community, ids in ascending old id"""
    comm = np.asarray(comm, dtype=np.int64)
    used = np.unique(comm)
    lab = np.searchsorted(used, comm)
    n2 = len(used)
    k2, in2 = np.zeros(n2, dtype=np.int64), np.zeros(n2, dtype=np.int64)
    np.add.at(k2, lab, lv.k)
    np.add.at(in2, lab, lv.inn)
    ls, ld = lab[lv.src], lab[lv.dst]
    inner = ls == ld
    np.add.at(in2, ls[inner], lv.a[inner])                            # both directions are listed: an inner edge adds 2 a
    if (~inner).any():
        o, keys, starts = _segments(ls[~inner] * n2 + ld[~inner])
        a2 = np.add.reduceat(lv.a[~inner][o], starts)
        src2, dst2 = keys // n2, keys % n2
    else:
        src2 = dst2 = a2 = np.zeros(0, dtype=np.int64)
    return Level(n2, src2, dst2, a2, k2, in2), lab


def modularity(sum_in, sum_d2, two_m, gamma):
    """from exact Python integers, every conversion rounding to nearest; 0 if 2m == 0"""
    if two_m == 0:
        return 0.0
    m2 = float(two_m)
    return float(sum_in) / m2 - float(gamma) * (float(sum_d2) / (m2 * m2))


def level_q(lv, two_m, gamma):
    return modularity(sum(lv.inn.tolist()), sum(x * x for x in lv.k.tolist()), two_m, gamma)


def label_q(lv0, two_m, labels, gamma):
    """the modularity of any labelling of the level-0 nodes"""
    _, lab = np.unique(np.asarray(labels), return_inverse=True)
    return level_q(aggregate(lv0, lab)[0], two_m, gamma)


def components(lv0, part):
    """per node the smallest node id of its connected component inside its part"""
    part = np.asarray(part)
    inner = part[lv0.src] == part[lv0.dst]
    s, d = lv0.src[inner], lv0.dst[inner]
    lab = np.arange(lv0.n, dtype=np.int64)
    while True:
        new = lab.copy()
        np.minimum.at(new, s, lab[d])
        while True:
            j = new[new]
            if np.array_equal(j, new):
                break
            new = j
        if np.array_equal(new, lab):
            return lab
        lab = new


def finish(lv0, part, split):
    """labels 1 .. C by descending node count, ties by smallest member id"""
    comp = components(lv0, part) if split else np.asarray(part)
    _, first, inv, cnt = np.unique(comp, return_index=True, return_inverse=True, return_counts=True)
    order = np.lexsort((first, -cnt))
    rank = np.empty(len(order), dtype=np.int64)
    rank[order] = np.arange(len(order))
    return (rank[inv] + 1).astype(np.int32), len(order)


def louvain(ptr, nbr, w, resolution=1.0, seed=4466, weight_scale=10000, max_sweeps=128, max_levels=32, split=True):
    """(labels int32 [n] in 1 .. C, {"q", "n_clusters", "two_m", "history": [(n, n', sweeps, moved, Q)]})"""
    lv0, two_m = level0(ptr, nbr, w, weight_scale)
    lv, map0 = lv0, np.arange(lv0.n, dtype=np.int64)
    cur_q = best_q = level_q(lv0, two_m, resolution)
    best, history = map0, []
    for level in range(max_levels):
        comm, sweeps, moved = phase(lv, resolution, two_m, seed, level, max_sweeps)
        if moved == 0:
            history.append((lv.n, lv.n, sweeps, 0, cur_q))
            break
        nx, lab = aggregate(lv, comm)
        map0 = lab[map0]
        cur_q = level_q(nx, two_m, resolution)
        history.append((lv.n, nx.n, sweeps, moved, cur_q))
        if cur_q > best_q:
            best_q, best = cur_q, map0
        lv = nx
    labels, C = finish(lv0, best, split)
    return labels, {"q": label_q(lv0, two_m, labels, resolution), "n_clusters": C, "two_m": two_m, "history": history}


# ---- graphs --------------------------------------------------------------------------------------------------------
def csr_of_edges(n, edges):
    """edges: (i, j, w) in listing order, each listed once from i; rows keep that order"""
    rows = [[] for _ in range(n)]
    for i, j, x in edges:
        rows[i].append((j, x))
    ptr = np.zeros(n + 1, dtype=np.int64)
    ptr[1:] = np.cumsum([len(r) for r in rows])
    nbr = np.array([j for r in rows for j, _ in r], dtype=np.int64)
    w = np.array([x for r in rows for _, x in r], dtype=np.float64)
    return ptr, nbr, w


def clique(n0, m, w=1.0):
    return [(n0 + i, n0 + j, w) for i in range(m) for j in range(i + 1, m)]


def tiny_graphs():
    """name -> (ptr, nbr, w): the graphs whose answer is known"""
    g = {}
    g["two_k4_bridge"] = csr_of_edges(8, clique(0, 4) + clique(4, 4) + [(3, 4, 1.0)])
    g["ring12"] = csr_of_edges(12, [(i, (i + 1) % 12, 1.0) for i in range(12)])
    g["k2"] = csr_of_edges(2, [(0, 1, 1.0)])
    g["star9"] = csr_of_edges(9, [(0, i, 1.0) for i in range(1, 9)])
    g["k55"] = csr_of_edges(10, [(i, 5 + j, 1.0) for i in range(5) for j in range(5)])
    g["loops_and_isolated"] = csr_of_edges(6, [(0, 0, 1.0), (2, 2, 0.5), (5, 5, 0.25)])
    return g


def hubs_graph(lengths, pool=200, seed=3):
    """one hub per entry of `lengths` with exactly that many neighbours, drawn from a weighted ring of `pool` leaves"""
    rng = np.random.default_rng(seed)
    n = pool + len(lengths)
    edges = [(i, (i + 1) % pool, round(float(rng.integers(1, 101)) / 100, 2)) for i in range(pool)]
    for h, L in enumerate(lengths):
        for j in rng.choice(pool, size=L, replace=False).tolist():
            edges.append((n - len(lengths) + h, j, round(float(rng.integers(1, 101)) / 100, 2)))
    return csr_of_edges(n, edges)


def many_hubs_graph(hubs, leaves, seed=3):
    """`hubs` hubs, each joined to every one of `leaves` leaves; the leaves sit on a ring; every weight is
    integers(1, 101) / 100.  The hubs are the last nodes"""
    rng = np.random.default_rng(seed)
    edges = [(i, (i + 1) % leaves, round(float(rng.integers(1, 101)) / 100, 2)) for i in range(leaves)]
    edges += [(leaves + h, j, round(float(rng.integers(1, 101)) / 100, 2)) for h in range(hubs) for j in range(leaves)]
    return csr_of_edges(leaves + hubs, edges)


def capacity_graphs(cap):
    """name -> (ptr, nbr, w): the graphs made for the sweep's table of `cap` distinct neighbour communities
    (tests/test_community_gpu.py runs them, tests/test_community_cpu.py asserts what their rows hold)"""
    return {"many_over_capacity": many_hubs_graph(20, cap + 40),
            "hubs_capacity": hubs_graph([cap - 1, cap, cap + 1], pool=cap + 40),
            "hubs_long_fit": hubs_graph([257, 600, 1500], pool=1600)}


CAPACITY_GRAPHS = ("many_over_capacity", "hubs_capacity", "hubs_long_fit")


def distinct_neighbour_communities(lv, comm, rows):
    """per row of `rows` the number of distinct communities among its neighbours j != i"""
    comm = np.asarray(comm)
    return [len(set(comm[lv.dst[lv.src == i]].tolist())) for i in rows]


def check_capacity_graph(name, lv, two_m, long_threshold, cap, seed, workgroup=256):
    """asserts that a graph of capacity_graphs meets the path it was made for: the hubs' row lengths and, from the
    yardstick's own trace, how many distinct neighbour communities they have in the sweeps that matter.  `workgroup`:
    the lanes of the long path's workgroup (CM_THREADS in nabo_amd/csrc/community.hip)"""
    rows = np.bincount(lv.src, minlength=lv.n)
    if name == "many_over_capacity":
        hubs = list(range(lv.n - 20, lv.n))
        assert rows[-20:].tolist() == [cap + 40] * 20 and rows[:-20].max() <= long_threshold
        trace = []
        phase(lv, 1.0, two_m, seed, 0, trace=trace)
        assert len(trace) >= 2
        # sweep 0: 20 rows beyond the table, on 8 workgroups: every dense table is used two or three times
        assert distinct_neighbour_communities(lv, trace[0][0], hubs) == [cap + 40] * 20
        # sweep 1: the same rows fit the table, at 91 % load
        d1 = distinct_neighbour_communities(lv, trace[1][0], hubs)
        assert d1 == [1862] * 20 and 0.9 * cap < d1[0] <= cap
    elif name == "hubs_capacity":                            # from singletons: one under, at and one over a full table
        want = [cap - 1, cap, cap + 1]
        assert rows[-3:].tolist() == want and rows[:-3].max() <= long_threshold
        assert distinct_neighbour_communities(lv, np.arange(lv.n), [lv.n - 3, lv.n - 2, lv.n - 1]) == want
    elif name == "hubs_long_fit":                            # more arcs than the workgroup has lanes, and they fit the table
        assert rows[-3:].tolist() == [257, 600, 1500] and rows[:-3].max() <= long_threshold
        assert workgroup < 257 and 2 * workgroup < 600 and 1500 < cap
    else:
        raise KeyError(name)


def blob_snn_graph(n=3000, centres=8, dims=10, k=11, seed=0):
    """Nabo's SNN graph of Gaussian blobs: every cell lists its k nearest cells (itself included), an edge weighs
    round(s / (2 (k - 1) - s), 2), s the neighbours both ends share (nabo/_mapping.py:185-198)"""
    rng = np.random.default_rng(seed)
    c = rng.normal(size=(centres, dims)) * 4.0
    X = c[rng.integers(0, centres, size=n)] + rng.normal(size=(n, dims))
    d2 = (X * X).sum(1)[:, None] - 2.0 * (X @ X.T) + (X * X).sum(1)[None, :]
    np.fill_diagonal(d2, -1.0)
    idx = np.argsort(d2, axis=1, kind="stable")[:, :k]
    member = np.zeros((n, n), dtype=bool)
    member[np.arange(n)[:, None], idx] = True
    edges = []
    factor = 2 * (k - 1)
    for i in range(n):
        for j in sorted(idx[i].tolist()):
            s = int((member[i] & member[j]).sum())
            if s > 0:
                edges.append((i, j, round(s / (factor - s), 2)))
    return csr_of_edges(n, edges)


def reference_loops_q(ptr, nbr, w, labels):
    """Graph.calc_modularity (nabo/_graph.py:415-442) restated loop for loop in Python floats on the simple graph with its
    float weights: (q, the number of float additions its sums made, the largest number of edges at a node)"""
    ptr, nbr, w = np.asarray(ptr), np.asarray(nbr), np.asarray(w, dtype=np.float64)
    n = len(ptr) - 1
    adj = [dict() for _ in range(n)]
    for i in range(n):
        for e in range(int(ptr[i]), int(ptr[i + 1])):
            j = int(nbr[e])
            adj[i][j] = adj[j][i] = float(w[e])
    w_degree, size, adds = [], 0.0, 0
    for i in range(n):
        d = 0.0
        for j, x in adj[i].items():
            d += 2 * x if j == i else x                     # networkx: a self-loop counts twice in the degree
            adds += 1
        w_degree.append(d)
    for i in range(n):
        for j, x in adj[i].items():
            if j >= i:
                size += x
                adds += 1
    norm = 1 / (2 * size)
    partition = {}
    for i, v in enumerate(np.asarray(labels).tolist()):
        partition.setdefault(v, {})[i] = None
    q = 0
    for p in partition.values():
        for i in p:
            t = -w_degree[i] * norm
            q += sum([t * w_degree[x] for x in p])
            q += sum([adj[i][x] for x in adj[i] if x in p])
            adds += len(p) + sum(1 for x in adj[i] if x in p) + 2
    return q * norm, adds, max(len(a) for a in adj)


def loops_bound(adds, max_edges):
    """|reference_loops_q - the exact Q| is at most this.  The loops add `adds` floats; a recursive sum of N terms errs by
    at most N u times the sum of the terms' magnitudes (u = 2^-53, first order).  Every term carries the rounding of its
    own operations on top: a degree is a sum of up to max_edges weights, each held to u (hundredths are not binary
    fractions), so it is good to (max_edges + 1) u; a product t * w_x holds two degrees, norm (good to (adds + 2) u,
    counted in `adds` already through size) and three roundings.  After the final * norm the magnitudes add up to at most
    sum_c d_c^2 / (2m)^2 + sum_c in_c / 2m <= 2.  A factor 2 covers the second-order terms."""
    return 2.0 * 2.0 * float(adds + 2 * (max_edges + 1) + 5) * 2.0 ** -53
