"""Plain-Python / numpy hop-distance oracle for the path tests (no GPU): breadth-first search from one node at a time
on the undirected simple graph a CSR describes, as networkx's shortest_path_length does on the reference's refG."""
import numpy as np


def undirected(n, ptr, nbr):
    """(uptr, ucol): both directions of every arc, duplicates merged, self-loops kept"""
    ptr, nbr = np.asarray(ptr, dtype=np.int64), np.asarray(nbr, dtype=np.int64)
    src = np.repeat(np.arange(n, dtype=np.int64), np.diff(ptr))
    key = np.unique(np.concatenate([src * n + nbr, nbr * n + src]))
    u, v = key // n, key % n
    uptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(u, minlength=n), out=uptr[1:])
    return uptr, v


def bfs(uptr, ucol, s, wanted=None):
    """hop distances from s (-1: unreachable); with `wanted` (node ids) it may stop once all of them are reached"""
    n = uptr.shape[0] - 1
    dist = np.full(n, -1, dtype=np.int64)
    dist[s] = 0
    front = np.array([s], dtype=np.int64)
    left = None if wanted is None else set(int(w) for w in wanted) - {int(s)}
    level = 0
    while front.size and (left is None or left):
        level += 1
        deg = uptr[front + 1] - uptr[front]
        idx = np.repeat(uptr[front] - np.concatenate([[0], np.cumsum(deg)[:-1]]), deg) + np.arange(int(deg.sum()))
        nb = np.unique(ucol[idx])
        nb = nb[dist[nb] < 0]
        dist[nb] = level
        front = nb
        if left is not None:
            left -= set(nb.tolist())
    return dist


def pair_hops(uptr, ucol, members):
    """every pair i < j of the member list, in (i, j) lexicographic order"""
    members = [int(x) for x in members]
    out = []
    for i, a in enumerate(members[:-1]):
        d = bfs(uptr, ucol, a, members[i + 1:])
        out.extend(int(d[b]) for b in members[i + 1:])
    return out


def group_hops(uptr, ucol, grp_ptr, members):
    """(sum, unreached, pair distances) as nabo_refgraph_group_hops returns them"""
    s, u, ph = [], [], []
    for g in range(len(grp_ptr) - 1):
        d = pair_hops(uptr, ucol, members[grp_ptr[g]:grp_ptr[g + 1]])
        s.append(sum(x for x in d if x >= 0))
        u.append(sum(1 for x in d if x < 0))
        ph.extend(d)
    return np.array(s, dtype=np.int64), np.array(u, dtype=np.int64), np.array(ph, dtype=np.int32)


def mapped_sets(t_ptr, t_nbr):
    gp, mem = [0], []
    for i in range(len(t_ptr) - 1):
        mem.extend(dict.fromkeys(int(x) for x in t_nbr[t_ptr[i]:t_ptr[i + 1]]))
        gp.append(len(mem))
    return gp, mem


def specificity(uptr, ucol, t_ptr, t_nbr, fill_na):
    """mapping specificity values in target-node order, as the reference computes them"""
    gp, mem = mapped_sets(t_ptr, t_nbr)
    vals = []
    for g in range(len(gp) - 1):
        d = pair_hops(uptr, ucol, mem[gp[g]:gp[g + 1]])
        if any(x < 0 for x in d):
            raise ValueError("unreachable pair")
        vals.append(float(np.mean(d)) if d else float("nan"))
    if fill_na:
        top = max(vals)
        if top == top:
            vals = [top if v != v else v for v in vals]
    return vals
