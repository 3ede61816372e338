"""numpy / Python-int restatement of include/nabo_agglom.h, the yardstick of the agglomeration tests: the gain of a pair,
one locally dominant pass, a round's matching by passes and by the sequential greedy walk, the whole run with its
dendrogram, and the cut.  Built on tests/_community_ref.py (level0, aggregate, modularity, finish); every gain is a Python
integer, so nothing here rounds.  Nothing is shared with the device code."""
import numpy as np

import _community_ref as cr


def gains(lv, two_m):
    """D(c, d) = a_cd 2m - k_c k_d of every arc of the level, as Python integers (an object array)"""
    return lv.a.astype(object) * int(two_m) - lv.k[lv.src].astype(object) * lv.k[lv.dst].astype(object)


def match_pass(lv, two_m, free=None, any_sign=False):
    """one pass: (partner int64 [n], -1 for none; D object [n], 0 for none; a int64 [n], the arc's weight, 0 for none).
    Every free c picks, among its free neighbours d with D(c, d) > 0 (any D with any_sign), the pair first in pair order:
    D descending, then the lower id of the pair ascending, then the higher."""
    n = lv.n
    free = np.ones(n, dtype=bool) if free is None else np.asarray(free).astype(bool)
    partner, D, a = np.full(n, -1, dtype=np.int64), np.zeros(n, dtype=object), np.zeros(n, dtype=np.int64)
    if len(lv.src) == 0:
        return partner, D, a
    g = gains(lv, two_m)
    ok = free[lv.src] & free[lv.dst]
    if not any_sign:
        ok &= np.array([x > 0 for x in g.tolist()], dtype=bool)
    at = np.flatnonzero(ok)
    if at.size == 0:
        return partner, D, a
    src, dst = lv.src[at], lv.dst[at]
    # D = hi 2^64 + lo with 0 <= lo < 2^64 and |hi| < 2^42: (hi, lo) in dictionary order is the order of the integers
    hi = np.array([x >> 64 for x in g[at].tolist()], dtype=np.int64)
    lo = np.array([x & cr.M64 for x in g[at].tolist()], dtype=np.uint64)
    o = np.lexsort((np.maximum(src, dst), np.minimum(src, dst), ~lo, -hi, src))
    first = o[np.flatnonzero(np.r_[True, src[o][1:] != src[o][:-1]])]
    partner[src[first]] = dst[first]
    D[src[first]] = g[at][first]
    a[src[first]] = lv.a[at][first]
    return partner, D, a


def pair_order(pairs):
    """pairs (c, d, D, a) with c < d in pair order"""
    return sorted(pairs, key=lambda p: (-p[2], p[0], p[1]))


def greedy_matching(lv, two_m):
    """the definition, sequentially: walk the pairs with D > 0 in pair order and take a pair if both ends are free"""
    g = gains(lv, two_m).tolist()
    pairs = [(int(c), int(d), x, int(a)) for c, d, x, a in zip(lv.src.tolist(), lv.dst.tolist(), g, lv.a.tolist()) if c < d and x > 0]
    free, taken = np.ones(lv.n, dtype=bool), []
    for c, d, x, a in pair_order(pairs):
        if free[c] and free[d]:
            free[c] = free[d] = False
            taken.append((c, d, x, a))
    return taken


def first_pair(lv, two_m):
    """the single first pair of the order among ALL pairs, whatever the sign of D (None without an arc)"""
    g = gains(lv, two_m).tolist()
    pairs = [(int(c), int(d), x, int(a)) for c, d, x, a in zip(lv.src.tolist(), lv.dst.tolist(), g, lv.a.tolist()) if c < d]
    return pair_order(pairs)[0] if pairs else None


def match(lv, two_m):
    """one round's matching by passes: (pairs (c, d, D, a) in pair order, passes, trace); trace holds per pass
    (clusters that picked a partner, pairs matched).  `passes` counts every pass run, the one that matched nothing
    included; the round without a positive gain takes the first pair of the order, found by one pass more over every
    sign, which is not counted."""
    free = np.ones(lv.n, dtype=bool)
    pairs, passes, trace = [], 0, []
    while True:
        p, D, a = match_pass(lv, two_m, free)
        passes += 1
        c = np.flatnonzero(p >= 0)
        lead = c[(p[p[c]] == c) & (c < p[c])]
        trace.append((int(c.size), int(lead.size)))
        if lead.size == 0:
            break
        pairs += [(int(x), int(p[x]), D[x], int(a[x])) for x in lead.tolist()]
        free[lead] = False
        free[p[lead]] = False
    if not pairs and len(lv.src):
        p, D, a = match_pass(lv, two_m, None, any_sign=True)
        c = np.flatnonzero(p >= 0)
        best = pair_order([(min(int(x), int(p[x])), max(int(x), int(p[x])), D[x], int(a[x])) for x in c.tolist()])[0]
        pairs = [best]
    return pair_order(pairs), passes, trace


def comm_of(n, pairs):
    comm = np.arange(n, dtype=np.int64)
    for c, d, _, _ in pairs:
        comm[d] = c
    return comm


def run(ptr, nbr, w, n_min=1, weight_scale=10000, levels=None):
    """the whole run from level 0: {"merges": int64 [M, 6] (rep_a, rep_b, round, a_cd, k_a, k_b), "rounds", "passes",
    "q_path": float64 [M + 1], "x_path": the exact integers sum_in 2m - sum_d2 (Python ints), "peak", "n_end", "lv0",
    "two_m"}; levels: a list that receives (level, pairs, passes) of every round"""
    lv0, two_m = cr.level0(ptr, nbr, w, weight_scale)
    lv, rep = lv0, np.arange(lv0.n, dtype=np.int64)
    merges, rounds, passes = [], 0, 0
    while lv.n > n_min and len(lv.src):
        pairs, p, _ = match(lv, two_m)
        passes += p
        take = min(len(pairs), lv.n - n_min)
        if levels is not None:
            levels.append((lv, pairs, p))
        merges += [(int(rep[c]), int(rep[d]), rounds, a, int(lv.k[c]), int(lv.k[d])) for c, d, _, a in pairs[:take]]
        comm = comm_of(lv.n, pairs[:take])
        rep = rep[comm == np.arange(lv.n)]
        lv = cr.aggregate(lv, comm)[0]
        rounds += 1
        if take < len(pairs):
            break
    si, sd = sum(lv0.inn.tolist()), sum(x * x for x in lv0.k.tolist())
    x_path, q_path = [si * two_m - sd], [cr.modularity(si, sd, two_m, 1.0)]
    for _, _, _, a, ka, kb in merges:
        si += 2 * a
        sd += 2 * ka * kb
        x_path.append(si * two_m - sd)
        q_path.append(cr.modularity(si, sd, two_m, 1.0))
    return {"merges": np.array(merges, dtype=np.int64).reshape(-1, 6), "rounds": rounds, "passes": passes,
            "q_path": np.array(q_path, dtype=np.float64), "x_path": x_path, "peak": x_path.index(max(x_path)), "n_end": lv.n,
            "lv0": lv0, "two_m": two_m}


def cut(res, n_clusters):
    """(labels int32 1 .. C by size, C, Q) after the first n0 - n_clusters merges; n_clusters = 0: the peak"""
    n0 = res["lv0"].n
    t = res["peak"] if n_clusters == 0 else n0 - n_clusters
    if t < 0 or t > len(res["merges"]):
        raise ValueError("n_clusters=%d is outside [%d, %d]" % (n_clusters, res["n_end"], n0))
    parent = np.arange(n0, dtype=np.int64)
    parent[res["merges"][:t, 1]] = res["merges"][:t, 0]
    while True:
        j = parent[parent]
        if np.array_equal(j, parent):
            break
        parent = j
    labels, C = cr.finish(res["lv0"], parent, False)
    return labels, C, float(res["q_path"][t])
