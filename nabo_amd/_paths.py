"""Hop distances on the reference graph: mapping specificity and contiguous path lengths on the GPU.

Array / HDF5 restatement of three methods of the reference's `Graph` (nabo/_graph.py) that call networkx's
`shortest_path_length` once per node pair on `refG`, the reference's SNN graph as an undirected simple graph:

  * `get_mapping_specificity` (:794-824)  per target node, the mean hop distance over all pairs of the reference
    nodes it is connected to;
  * `get_ref_specificity`     (:826-857)  per reference node, the mean specificity of the target nodes mapped to it;
  * `calc_contiguous_spl`     (:904-916)  the mean hop distance between consecutive nodes of a list.

The distances come from `nabo_refgraph_group_hops` (include/nabo_graph.h, nabo_amd/csrc/paths.hip): every pair
of a group of reference nodes, answered by a workgroup-local search or by whole-graph multi-source BFS sweeps.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._graphio import csr_by_node_id, open_ref as _open_ref


def _i64(a, name):
    a = np.ascontiguousarray(a, dtype=np.int64)
    if a.ndim != 1:
        raise ValueError("ERROR: %s must be 1-D" % name)
    return a


class _DeviceGraph:
    """A graph resident on one device (nabo_refgraph_create); node ids are 0 .. n-1."""

    def __init__(self, ptr, nbr, device=0, options=None):
        ptr, nbr = _i64(ptr, "ptr"), _i64(nbr, "nbr")
        if ptr.shape[0] < 1:
            raise ValueError("ERROR: ptr needs n_nodes + 1 entries")
        if int(ptr[-1]) != nbr.shape[0]:
            raise ValueError("ERROR: ptr[-1] = %d but nbr has %d entries" % (int(ptr[-1]), nbr.shape[0]))
        self.n = ptr.shape[0] - 1
        self._h = None
        L = _lib.lib()
        h = C.c_void_p()
        _lib.check(L.nabo_refgraph_create(C.byref(h), int(device), int(self.n), ptr.ctypes.data, nbr.ctypes.data))
        self._h = h
        for k, v in (options or {}).items():
            self.set_option(k, v)

    def set_option(self, name, value):
        _lib.check(_lib.lib().nabo_refgraph_set_option(self._h, name.encode(), int(value)))

    def group_hops(self, grp_ptr, members, pair_hops=False):
        grp_ptr, members = _i64(grp_ptr, "grp_ptr"), _i64(members, "members")
        if grp_ptr.shape[0] < 1 or int(grp_ptr[-1]) != members.shape[0]:
            raise ValueError("ERROR: grp_ptr must have n_groups + 1 entries ending at len(members)")
        G = grp_ptr.shape[0] - 1
        m = np.diff(grp_ptr)
        if (m < 0).any():
            raise ValueError("ERROR: grp_ptr is not monotone")
        s = np.zeros(G, dtype=np.int64)
        u = np.zeros(G, dtype=np.int64)
        ph = np.empty(int((m * (m - 1) // 2).sum()), dtype=np.int32) if pair_hops else None
        _lib.check(_lib.lib().nabo_refgraph_group_hops(self._h, int(G), grp_ptr.ctypes.data, members.ctypes.data,
                                                       s.ctypes.data, u.ctypes.data, None if ph is None else ph.ctypes.data))
        return (s, u, ph) if pair_hops else (s, u)

    def set_levels(self, set_ptr, members, max_level=-1):
        """int32 [n_sets, n]: hops from every node to the nearest member of each set (nabo_refgraph_set_levels,
        include/nabo_cluster.h); -1 = unreachable or beyond max_level (max_level < 0: no limit)"""
        set_ptr, members = _i64(set_ptr, "set_ptr"), _i64(members, "members")
        if set_ptr.shape[0] < 1 or int(set_ptr[-1]) != members.shape[0]:
            raise ValueError("ERROR: set_ptr must have n_sets + 1 entries ending at len(members)")
        S = set_ptr.shape[0] - 1
        out = np.empty((S, self.n), dtype=np.int32)
        _lib.check(_lib.lib().nabo_refgraph_set_levels(self._h, int(S), set_ptr.ctypes.data, members.ctypes.data,
                                                       int(max_level), out.ctypes.data))
        return out

    def last_stats(self):
        """{"ms": (build, local, global, total), "local_groups", "global_groups", "sweeps", "max_level"}"""
        ms = (C.c_double * 4)()
        cnt = (C.c_int64 * 4)()
        _lib.check(_lib.lib().nabo_refgraph_last_stats(self._h, ms, cnt))
        return {"ms": tuple(ms), "local_groups": cnt[0], "global_groups": cnt[1], "sweeps": cnt[2], "max_level": cnt[3]}

    def last_local_nodes(self, n_groups):
        out = np.empty(int(n_groups), dtype=np.int32)
        _lib.check(_lib.lib().nabo_refgraph_last_local_nodes(self._h, int(n_groups), out.ctypes.data))
        return out

    def close(self):
        if self._h is not None:
            _lib.lib().nabo_refgraph_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def group_hops(ptr, nbr, grp_ptr, members, pair_hops=False, device=0, options=None):
    """Hop distances of every member pair of every group, on the undirected simple graph a CSR (ptr, nbr) describes
    (rows in either arc direction; duplicate arcs and self-loops allowed).

    Group g is members[grp_ptr[g]:grp_ptr[g+1]] (node ids; repeats allowed, a repeated pair is at distance 0).
    Returns (sum, unreached): int64 [n_groups] sums of the reachable pairs' distances and counts of unreachable
    pairs; with pair_hops=True also int32 distances of every pair (-1 = no path), each group's m(m-1)/2 pairs in
    (i, j) lexicographic order, groups one after the other.  `options`: {"local_capacity": .., "local_max_members":
    ..} (include/nabo_graph.h) -- they decide which tier answers a group, never the result."""
    g = _DeviceGraph(ptr, nbr, device, options)
    try:
        return g.group_hops(grp_ptr, members, pair_hops)
    finally:
        g.close()


# ---- the mapping file ---------------------------------------------------------------------------------------------
def _ref_nodes_in_file_order(h5, ref_uid):
    """Graph.refNodes: the reference's nodes as load_from_h5 meets them (HDF5 name order of its graph group; the
    columnar layout lists them in that order too, see read_graph_csr)"""
    from ._mapping import _G_NODES, _G_PTR
    grp = h5[ref_uid + "_graph"]
    if _G_PTR in grp:
        return sorted(x.decode("UTF-8") for x in grp[_G_NODES][:])
    return [n for n in grp]


def _target_rows_w(h5, target, pos):
    """(target node names in load order, ptr, reference positions, weights) of one mapped sample; KeyError if absent"""
    from ._mapping import read_graph_csr
    uid = None
    if "target_names" in h5["name_stash"]:
        for i in h5["name_stash/target_names"][:]:
            if i[0].decode("UTF-8") == target:
                uid = i[1].decode("UTF-8")
    if uid is None:
        raise KeyError(target)
    return read_graph_csr(h5[uid + "_graph"], pos)


def _target_rows(h5, target, pos):
    """(target node names in load order, ptr, reference positions) of one mapped sample; KeyError if absent"""
    return _target_rows_w(h5, target, pos)[:3]


def _mapped_sets(ptr, nbr):
    """per target node, its reference neighbours once each in first-seen order (networkx adjacency order)"""
    gp, mem = [0], []
    for i in range(len(ptr) - 1):
        seen = dict.fromkeys(nbr[ptr[i]:ptr[i + 1]].tolist())
        mem.extend(seen)
        gp.append(len(mem))
    return np.array(gp, dtype=np.int64), np.array(mem, dtype=np.int64)


def _ref_specificity(h5, ref_name, target, target_values, incl_unmapped):
    names, pos, ref_uid = _open_ref(h5, ref_name)
    ref_nodes = _ref_nodes_in_file_order(h5, ref_uid)
    t_nodes, ptr, nbr = _target_rows(h5, target, pos)
    return _ref_specificity_rows(ref_nodes, pos, len(names), t_nodes, ptr, nbr, target_values, incl_unmapped)


def _ref_specificity_rows(ref_nodes, pos, n_ref, t_nodes, ptr, nbr, target_values, incl_unmapped):
    """ref_nodes: reference node names in the reference's node order; pos: name -> id; rows hold ids"""
    gp, mem = _mapped_sets(ptr, nbr)
    back = [[] for _ in range(n_ref)]
    for i, t in enumerate(t_nodes):
        for r in mem[gp[i]:gp[i + 1]].tolist():
            back[r].append(target_values[t])
    out = {}
    for n in ref_nodes:
        v = back[pos[n]]
        if len(v) > 1:
            out[n] = np.mean(v)
        elif len(v) == 1:
            out[n] = v[0]
        elif incl_unmapped:
            out[n] = 0
    return out


def _raise_unreachable(dg, names, grp_ptr, members, g):
    a0, a1 = int(grp_ptr[g]), int(grp_ptr[g + 1])
    mem = members[a0:a1]
    _, _, ph = dg.group_hops(np.array([0, a1 - a0], dtype=np.int64), mem, pair_hops=True)
    p = int(np.nonzero(ph < 0)[0][0])
    m, i = a1 - a0, 0
    while p >= m - i - 1:
        p -= m - i - 1
        i += 1
    raise ValueError("ERROR: no path between %s and %s in the reference graph" % (names[mem[i]], names[mem[i + 1 + p]]))


def _specificity(dg, names, t_nodes, ptr, nbr, fill_na):
    """mapping specificity of target nodes t_nodes whose rows (ptr, nbr) hold reference node ids of dg"""
    gp, mem = _mapped_sets(ptr, nbr)
    s, u = dg.group_hops(gp, mem)
    bad = np.nonzero(u)[0]
    if bad.size:
        _raise_unreachable(dg, names, gp, mem, int(bad[0]))
    m = np.diff(gp)
    pairs = m * (m - 1) // 2
    vals = [float(s[i]) / float(pairs[i]) if m[i] > 1 else float("nan") for i in range(len(t_nodes))]
    out = dict(zip(t_nodes, vals))
    if fill_na:
        top = max(out.values())
        if top == top:
            out = {k: (top if v != v else v) for k, v in out.items()}
    return out


def _contiguous(dg, names, idx):
    idx = np.asarray(idx, dtype=np.int64)
    if idx.shape[0] < 2:
        return float("nan")
    G = idx.shape[0] - 1
    gp = np.arange(0, 2 * G + 1, 2, dtype=np.int64)
    mem = np.stack([idx[:-1], idx[1:]], axis=1).reshape(-1)
    s, u = dg.group_hops(gp, mem)
    bad = np.nonzero(u)[0]
    if bad.size:
        _raise_unreachable(dg, names, gp, mem, int(bad[0]))
    return float(s.sum()) / float(G)


class RefGraph:
    """The reference graph of a mapping file, resident on the GPU, with the path methods of the reference's Graph.

    Reads the reference's `<uid>_graph` in either layout (per-node or columnar, `read_graph_csr`) and keeps the
    undirected simple graph networkx's `refG` would be on the device.  Node ids are positions in
    `ref_cells/ref_cells`; nodes are named `<cell>_<ref_name>` as in the reference.  Use as a context manager or
    call close()."""

    def __init__(self, mapping_h5_fn, ref_name, device=0, options=None):
        import h5py
        from ._mapping import read_graph_csr
        self.fn, self.ref_name, self.device, self.layout = mapping_h5_fn, ref_name, device, None
        with h5py.File(mapping_h5_fn, "r") as h5:
            self.names, self.pos, ref_uid = _open_ref(h5, ref_name)
            rows, ptr, nbr, _ = read_graph_csr(h5[ref_uid + "_graph"], self.pos)
        # rows in the group's order -> a CSR by reference position (arc direction does not matter to the device)
        cptr, cnbr, _ = csr_by_node_id(rows, self.pos, len(self.names), ptr, nbr)
        self.ref_nodes = list(rows)      # Graph.refNodes: read_graph_csr lists rows in the file's node order (either layout)
        self.selfloop = np.zeros(len(self.names), dtype=bool)
        self.selfloop[cnbr[cnbr == np.repeat(np.arange(len(self.names)), np.diff(cptr))]] = True
        self.deTestCells, self.deCtrlCells = None, None
        self._g = _DeviceGraph(cptr, cnbr, device, options)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def close(self):
        if getattr(self, "_g", None) is not None:
            self._g.close()
            self._g = None
        if getattr(self, "_agglom", None) is not None:
            self._agglom[2].close()
            self._agglom = None

    def last_stats(self):
        return self._g.last_stats()

    def mapping_specificity(self, target_name, fill_na=True):
        """Graph.get_mapping_specificity (nabo/_graph.py:794-824): {target node: mean hop distance over all pairs of
        the reference nodes it is connected to}.  Matches the reference bit for bit, quirks included:

          * the value is float64(sum of pair distances) / float64(number of pairs) -- equal to the reference's
            float(np.mean(spls)), whose sum of integers is exact;
          * a target node with fewer than 2 mapped reference nodes gets NaN;
          * keys follow the target's node order in the file (HDF5 name order, `load_from_h5` :93-107);
          * fill_na replaces NaN by Python's max(values): if the FIRST value is NaN that maximum is NaN and nothing is
            filled; a target with no nodes raises ValueError as max() of nothing does;
          * an unreachable pair raises ValueError naming both nodes (the reference raises networkx.NetworkXNoPath);
          * an unknown target raises KeyError."""
        import h5py
        with h5py.File(self.fn, "r") as h5:
            t_nodes, ptr, nbr = _target_rows(h5, target_name, self.pos)
        return _specificity(self._g, self.names, t_nodes, ptr, nbr, fill_na)

    def ref_specificity(self, target, target_values, incl_unmapped=False):
        """Graph.get_ref_specificity (nabo/_graph.py:826-857): {reference node: mean of target_values over the nodes
        of `target` mapped to it}.  Keys in the reference's node order (the file's); each node's values in the order
        networkx lists its neighbours (the target's node order), so the mean is np.mean of the same list, bit for bit;
        a node with one mapped target node gets that value as is, one with none is left out (or 0 with
        incl_unmapped).  A target node missing from target_values raises KeyError.  The reference selects neighbours
        whose NAME ends with `target`, so a reference neighbour or another sample's node named that way would also
        be picked up; here only the nodes of sample `target` count.  Host code: no GPU is used."""
        import h5py
        with h5py.File(self.fn, "r") as h5:
            return _ref_specificity(h5, self.ref_name, target, target_values, incl_unmapped)

    def contiguous_spl(self, nodes):
        """Graph.calc_contiguous_spl (nabo/_graph.py:904-916): mean hop distance between consecutive nodes of the list
        (node names).  Fewer than 2 nodes give NaN (np.mean of nothing); an unknown node raises KeyError; an
        unreachable pair raises ValueError (the reference: networkx.NodeNotFound / NetworkXNoPath)."""
        return _contiguous(self._g, self.names, [self.pos[n] for n in nodes])

    def k_path_neighbours(self, nodes, k_dist, full_trail=False, trail_start=0):
        """Graph.get_k_path_neighbours (nabo/_graph.py:956-987): the reference nodes at exactly `k_dist` hops from the
        node list, or with full_trail the rings `1 + trail_start` .. `k_dist` one after the other.  The reference peels
        rings off a copy of the graph (quadratic in the ring size); here one multi-source sweep gives every node's hop
        level and the rings are read off it.  The list [list(nodes), ring 1, ..., ring k_dist] goes through the
        reference's own return expressions (`rings[-1]`, `sum(rings[1 + trail_start:], [])`), so k_dist = 0 returns the
        nodes as given, and trail_start >= k_dist or a negative trail_start behave as Python slices do.  Quirks kept:

          * names that are not reference nodes are ignored from ring 1 on (but returned as given for k_dist = 0);
          * a node with a SELF-LOOP appears again in the ring after its own: the reference removes the edges between
            DISTINCT nodes of a ring only.  (A node listed twice in `nodes` loses its self-loop: combinations() pairs it
            with itself.)
          * rings stop growing when the component is exhausted: empty lists, no error.

        The reference returns each ring in set order; here a ring is sorted by reference position."""
        from ._classify import _k_path_neighbours
        return _k_path_neighbours(self, nodes, k_dist, full_trail, trail_start)

    def set_ref_layout(self, niter=500, init_pos=None, seed=0, disable_rescaling=False, verbose=True, **params):
        """Graph.set_ref_layout (nabo/_graph.py:179-237): {reference node: (x, y)}, the ForceAtlas2 layout of the
        reference graph with the repulsion summed over every pair; `params` and everything else as in
        nabo_amd.set_ref_layout, which this calls on the object's file and device (the weighted graph is read again
        through read_graph_csr: the resident graph keeps no weights).  The result is also kept as `self.layout`."""
        from ._layout import _set_ref_layout
        self.layout = _set_ref_layout(self.fn, self.ref_name, niter, init_pos, seed, disable_rescaling, verbose, self.device, params)
        return self.layout

    def bundle_edges(self, layout=None, edge_min_weight=0, bundle_bw=0.1, bundle_decay=0.7, **params):
        """The bundled edges of the reference graph as `GraphPlot(draw_edges='ref', bundle_edges=True)` draws them:
        (points, offsets), as nabo_amd.bundle_edges, which this calls on the object's file and device.  `layout`: as
        there; None takes `self.layout`, which `set_ref_layout` keeps."""
        from ._bundle import bundle_edges
        if layout is None:
            layout = self.layout
        if layout is None:
            raise ValueError("ERROR: no layout: call set_ref_layout first or give one")
        return bundle_edges(self.fn, self.ref_name, layout, edge_min_weight, bundle_bw, bundle_decay, self.device, **params)

    def render(self, layout=None, clusters=None, **kwargs):
        """The picture of the reference graph `GraphPlot` draws, rasterised on the device: (image uint8 [H, W, 4], extent),
        as nabo_amd.plot_graph, which this calls on the object's file and device with GraphPlot's arguments in `kwargs`.
        `layout`: as there; None takes `self.layout`, which `set_ref_layout` keeps.  `clusters`: None takes
        `self.clusters` if `make_leiden_clusters` has set it; pass {} to colour by `vc` alone."""
        from ._render import plot_graph
        if layout is None:
            layout = self.layout
        if layout is None:
            raise ValueError("ERROR: no layout: call set_ref_layout first or give one")
        if clusters is None:
            clusters = getattr(self, "clusters", None)
        return plot_graph(self.fn, self.ref_name, layout, clusters or None, device=self.device, **kwargs)

    def make_leiden_clusters(self, resolution=1.0, random_seed=4466):
        """Graph.make_leiden_clusters (nabo/_graph.py:266-292): {reference node: str(cluster)}, as
        nabo_amd.make_leiden_clusters, which this calls on the object's file and device (the weighted graph is read again
        through read_graph_csr: the resident graph keeps no weights).  The result is also kept as `self.clusters`."""
        from ._community import make_leiden_clusters
        self.clusters = make_leiden_clusters(self.fn, self.ref_name, resolution, random_seed, self.device)
        return self.clusters

    def make_clusters(self, n_clusters):
        """Graph.make_clusters (nabo/_graph.py:247-264): {reference node: str(cluster)} with exactly `n_clusters`
        clusters, as nabo_amd.make_clusters.  As the reference keeps `_agglomDendrogram`, the first call runs the
        agglomeration and keeps its handle, so another `n_clusters` runs only the cut.  The result is also kept as
        `self.clusters`."""
        from ._community import Community, _clusters_of_graph, _ref_graph_csr
        if getattr(self, "_agglom", None) is None:
            ref_nodes, pos, _, ptr, nbr, w = _ref_graph_csr(self.fn, self.ref_name)
            H = Community(ptr, nbr, w, device=self.device)
            H.agglomerate()
            self._agglom = (ref_nodes, pos, H)
        self.clusters = _clusters_of_graph(*self._agglom, n_clusters)
        return self.clusters

    def calc_modularity(self, clusters=None):
        """Graph.calc_modularity (nabo/_graph.py:415-442) of `clusters`, by default those make_leiden_clusters kept; as
        nabo_amd.calc_modularity."""
        from ._community import calc_modularity
        clusters = getattr(self, "clusters", None) if clusters is None else clusters
        return calc_modularity(self.fn, self.ref_name, {} if clusters is None else clusters, self.device)

    def calc_diff_potential(self, r=None, tol=1e-10, max_iter=10000):
        """Graph.calc_diff_potential (nabo/_graph.py:918-954): {reference node: V}, the population-balance potential
        pinv(I - A/D) r of the unweighted reference graph, as nabo_amd.calc_diff_potential, which this calls on the
        object's file and device."""
        from ._potential import calc_diff_potential
        return calc_diff_potential(self.fn, self.ref_name, r, tol, max_iter, self.device)

    def set_de_groups(self, target, min_score, node_dist, from_clusters=None, full_trail=False, trail_start=1,
                      stringent_control=False, clusters=None):
        """Graph.set_de_groups (nabo/_graph.py:989-1055): 'Test' = reference nodes whose mapping score for `target` is
        >= min_score (`get_mapping_score(target, min_score=min_score, all_nodes=False)`, its errors pass through),
        limited to the clusters `from_clusters` if given (a list, else TypeError; labels compared as str; `clusters` is
        the dict Graph.import_clusters takes and is validated as in classify_target); 'Control' =
        k_path_neighbours(Test, node_dist, full_trail, trail_start), without the nodes that have a score when
        stringent_control; 'Other' = the rest.  A Test node stays Test when it is also in the ring.  Fewer than 5 Test
        nodes: the reference's warning and None.  Else {"de_group": {reference node: group} in the file's node order,
        "deTestCells": [...], "deCtrlCells": [...]} (cell names; Test in node order, Control in ring order), the two
        lists also kept as attributes of those names."""
        from ._classify import _set_de_groups
        res = _set_de_groups(self, target, min_score, node_dist, from_clusters, full_trail, trail_start, stringent_control, clusters)
        if res is not None:
            self.deTestCells, self.deCtrlCells = res["deTestCells"], res["deCtrlCells"]
        return res


def get_mapping_specificity(mapping_h5_fn, ref_name, target_name, fill_na=True, device=0):
    """Graph.get_mapping_specificity from the mapping file (`mapping_h5_fn, ref_name` stand for the Graph object);
    see RefGraph.mapping_specificity."""
    with RefGraph(mapping_h5_fn, ref_name, device) as g:
        return g.mapping_specificity(target_name, fill_na)


def get_ref_specificity(mapping_h5_fn, ref_name, target, target_values, incl_unmapped=False):
    """Graph.get_ref_specificity from the mapping file; see RefGraph.ref_specificity (host code, no GPU)."""
    import h5py
    with h5py.File(mapping_h5_fn, "r") as h5:
        return _ref_specificity(h5, ref_name, target, target_values, incl_unmapped)


def calc_contiguous_spl(mapping_h5_fn, ref_name, nodes, device=0):
    """Graph.calc_contiguous_spl from the mapping file; see RefGraph.contiguous_spl."""
    with RefGraph(mapping_h5_fn, ref_name, device) as g:
        return g.contiguous_spl(nodes)
