"""Classification of target cells into the reference's clusters, and the Test / Control groups for differential
expression, on the GPU.

Array / HDF5 restatement of four methods of the reference's `Graph` (nabo/_graph.py):

  * `classify_target`       (:722-792)   per target node, the weight its edges put into every cluster of reference
    nodes; the node takes the best cluster if that holds more than `weight_frac` of its total weight;
  * `get_k_path_neighbours` (:956-987)   the reference nodes at 1 .. k hops from a node list;
  * `set_de_groups`         (:989-1055)  Test = reference nodes with mapping score >= `min_score`, Control = a ring or
    trail around them;
  * `get_mapped_cells`      (:859-884)   the target cells connected to given reference cells (host code).

The sums and labels come from `nabo_classify_targets`, the hop levels from `nabo_refgraph_set_levels`
(include/nabo_cluster.h, nabo_amd/csrc/classify.hip and paths.hip).  The device steps are kept apart from the host
logic: the `_*_from_*` functions take the label / level arrays, so the logic is testable without a GPU.
"""
from collections import Counter

import numpy as np

from . import _lib
from ._paths import RefGraph, _i64, _mapped_sets, _open_ref, _ref_nodes_in_file_order, _target_rows_w


# ---- arrays -------------------------------------------------------------------------------------------------------
def classify_from_edges(ref_cluster, ptr, nbr, w, weight_frac=0.5, min_degree=2, min_weight=0.1, n_clusters=None, device=0):
    """Classify target nodes from their rows (nabo_classify_targets, include/nabo_cluster.h).

    ref_cluster[r]: cluster id of reference node r in [0, n_clusters), or -1 for none; target node t has the edges
    nbr[ptr[t]:ptr[t+1]] (reference positions) with weights w[...] in file order.  A neighbour repeated in a row is one
    edge at its first position with its last weight.  Returns {"label": int32 [n_targets] (-1 = not classified),
    "best": float64 weight of the best cluster, "total": float64 total weight, "counts": int64 [n_clusters + 1] nodes
    per label, the last entry for -1}.  Ties for the best cluster go to the lowest id."""
    ref_cluster = np.ascontiguousarray(ref_cluster, dtype=np.int32)
    ptr, nbr = _i64(ptr, "ptr"), _i64(nbr, "nbr")
    w = np.ascontiguousarray(w, dtype=np.float64)
    if ref_cluster.ndim != 1 or w.ndim != 1:
        raise ValueError("ERROR: ref_cluster and w must be 1-D")
    if ptr.shape[0] < 1 or nbr.shape != w.shape:
        raise ValueError("ERROR: ptr needs n_targets + 1 entries, nbr and w one entry per edge")
    if (np.diff(ptr) < 0).any() or int(ptr[0]) != 0:
        raise ValueError("ERROR: ptr must start at 0 and be monotone")
    if int(ptr[-1]) != nbr.shape[0]:
        raise ValueError("ERROR: ptr[-1] = %d but nbr has %d entries" % (int(ptr[-1]), nbr.shape[0]))
    if n_clusters is None:
        n_clusters = int(ref_cluster.max()) + 1 if ref_cluster.size else 0
    n_t = ptr.shape[0] - 1
    label = np.empty(n_t, dtype=np.int32)
    best, total = np.empty(n_t, dtype=np.float64), np.empty(n_t, dtype=np.float64)
    counts = np.zeros(max(int(n_clusters), 0) + 1, dtype=np.int64)
    _lib.check(_lib.lib().nabo_classify_targets(int(device), int(ref_cluster.shape[0]), ref_cluster.ctypes.data, int(n_clusters),
                                                int(n_t), ptr.ctypes.data, nbr.ctypes.data, w.ctypes.data, float(weight_frac),
                                                int(min_degree), float(min_weight), label.ctypes.data, best.ctypes.data,
                                                total.ctypes.data, counts.ctypes.data))
    return {"label": label, "best": best, "total": total, "counts": counts}


def _device_classify(ref_cluster, n_clusters, ptr, nbr, w, weight_frac, min_degree, min_weight, device=0):
    """the device step of classify_target: (label, counts)"""
    r = classify_from_edges(ref_cluster, ptr, nbr, w, weight_frac, min_degree, min_weight, n_clusters, device)
    return r["label"], r["counts"]


# ---- classify_target ----------------------------------------------------------------------------------------------
def _imported_clusters(ref_nodes, clusters):
    """Graph.clusters after Graph.import_clusters(clusters) (:334-356): values as str, unnamed reference nodes 'NA';
    without an import no node has a cluster"""
    if clusters is None:
        return {}
    return {n: str(clusters[n]) if n in clusters else "NA" for n in ref_nodes}


def _validate_clusters(cluster_dict):
    nclusts = len(set(cluster_dict.values()))
    if nclusts == 0:
        raise ValueError('ERROR: Calculate clusters first using "make_leiden_clusters" or import clusters using '
                         '"import_clusters"')
    elif nclusts == 1:
        raise ValueError("ERROR: Cannot classify targets when only one cluster is present in the graph")
    return True


def _cluster_ids(ref_nodes, pos, n_ref, cluster_dict):
    """(labels, ref_cluster): cluster ids in order of first appearance over the reference nodes in the file's node
    order, then the labels cluster_dict gives only to names that are no reference node (they can win nothing but are
    counted); ref_cluster by reference position, -1 = not a key of cluster_dict"""
    ids, labels = {}, []
    ref_cluster = np.full(n_ref, -1, dtype=np.int32)
    for n in ref_nodes:
        if n in cluster_dict:
            c = cluster_dict[n]
            if c not in ids:
                ids[c] = len(labels)
                labels.append(c)
            ref_cluster[pos[n]] = ids[c]
    for c in cluster_dict.values():
        if c not in ids:
            ids[c] = len(labels)
            labels.append(c)
    return labels, ref_cluster


def _classify_from_labels(t_nodes, label, counts, labels, na_label, ret_counts):
    """the reference's two return shapes from the device's label ids and counts"""
    if ret_counts:
        out = Counter()
        for i in np.nonzero(counts[:-1])[0].tolist():
            out[labels[i]] += int(counts[i])
        out[na_label] += int(counts[-1])
        for c in labels:
            if c not in out:
                out[c] = 0
        return out
    return dict(zip(t_nodes, [labels[i] if i >= 0 else na_label for i in label.tolist()]))


def _classify_rows(ref_nodes, pos, n_ref, t_nodes, ptr, nbr, w, weight_frac, min_degree, min_weight, cluster_dict, na_label,
                   ret_counts, classify=_device_classify):
    """classify_target on one target's rows; `classify` is the device step (ref_cluster, n_clusters, ptr, nbr, w,
    weight_frac, min_degree, min_weight) -> (label, counts)"""
    labels, ref_cluster = _cluster_ids(ref_nodes, pos, n_ref, cluster_dict)
    if not labels:
        # max() over no clusters (:777) at the first node that passes min_degree
        gp, _ = _mapped_sets(ptr, nbr)
        if (np.diff(gp) >= min_degree).any():
            raise ValueError("max() arg is an empty sequence")
        label = np.full(len(t_nodes), -1, dtype=np.int32)
        counts = np.array([len(t_nodes)], dtype=np.int64)
    else:
        label, counts = classify(ref_cluster, len(labels), ptr, nbr, w, weight_frac, min_degree, min_weight)
    return _classify_from_labels(t_nodes, label, counts, labels, na_label, ret_counts)


def classify_target(mapping_h5_fn, ref_name, target, weight_frac=0.5, min_degree=2, min_weight=0.1, cluster_dict=None,
                    na_label="NA", ret_counts=False, clusters=None, device=0):
    """Graph.classify_target (nabo/_graph.py:722-792) from the mapping file (`mapping_h5_fn, ref_name` stand for the
    Graph object): {target node: label of the cluster that holds more than `weight_frac` of the node's total edge
    weight, else na_label}, or with ret_counts the number of target nodes per label.  Equal to the reference bit for
    bit, quirks included:

      * `clusters` is the dict `Graph.import_clusters` takes ({reference node: cluster}): values become str and the
        reference nodes it does not name get 'NA' -- a real cluster, which collides with the default na_label exactly
        as in the reference (both count under one key).  `cluster_dict` is the reference's explicit argument: labels of
        any hashable type as given, nodes it does not name have no cluster (their edges count for the total only);
      * neither given: ValueError ("Calculate clusters first"); `clusters` with one label: ValueError (:404-413).  An
        explicit cluster_dict is not validated; an empty one raises ValueError at the first node that passes
        min_degree (the reference's max() of nothing);
      * an unknown target raises KeyError (`self.targetNodes[target]`);
      * a neighbour repeated in a node's row is one edge, at its first position, with its LAST weight (nx.add_edge);
        the degree counts distinct neighbours; degree < min_degree gives na_label;
      * total = float64 sum of all edge weights in row order; a cluster's weight = float64 sum in row order of the
        weights > min_weight (strict) of neighbours that have a cluster; label iff best > weight_frac * total (strict);
      * keys follow the target's node order in the file; ret_counts returns a Counter with every label and na_label,
        zeros included;
      * FIXED BY THIS BUILD: two clusters tied for best.  The reference's max() runs over a dict built from a Python
        set of labels, so its pick follows the process's string hashing; here the tie goes to the lowest cluster id,
        ids numbered by first appearance over the reference nodes in the file's node order.  A tie can decide a label
        only when weight_frac < 0.5 (up to rounding of the total)."""
    import h5py
    with h5py.File(mapping_h5_fn, "r") as h5:
        names, pos, ref_uid = _open_ref(h5, ref_name)
        ref_nodes = _ref_nodes_in_file_order(h5, ref_uid)
        if cluster_dict is None:
            cluster_dict = _imported_clusters(ref_nodes, clusters)
            _validate_clusters(cluster_dict)
        t_nodes, ptr, nbr, w = _target_rows_w(h5, target, pos)

    def step(*a):
        return _device_classify(*a, device=device)
    return _classify_rows(ref_nodes, pos, len(names), t_nodes, ptr, nbr, w, weight_frac, min_degree, min_weight, cluster_dict,
                          na_label, ret_counts, step)


# ---- rings around a node list -------------------------------------------------------------------------------------
def _rings_from_levels(level, selfloop, names, pos, nodes, k_dist):
    """[list(nodes), ring 1, ..., ring k_dist] as get_k_path_neighbours builds them (:978-983), rings as names sorted by
    reference position.  level: hops of every reference node from the nodes of the list (-1: beyond k_dist or
    unreachable); selfloop: bool per reference node."""
    level = np.asarray(level)
    rings = [list(nodes)]
    seeds = Counter(pos[x] for x in nodes if x in pos)
    twice = [p for p, c in seeds.items() if c > 1]
    for r in range(1, k_dist + 1):
        again = (level == r - 1) & selfloop
        if r == 1 and twice:
            again[twice] = False        # combinations() pairs a repeated node with itself: its self-loop is removed
        rings.append([names[i] for i in np.nonzero((level == r) | again)[0].tolist()])
    return rings


def _k_path_from_rings(rings, full_trail, trail_start):
    """the reference's two return expressions (:984-987)"""
    if full_trail:
        return sum(rings[1 + trail_start:], [])
    return rings[-1]


def _k_path_neighbours(graph, nodes, k_dist, full_trail, trail_start):
    nodes = list(nodes)
    seeds = [graph.pos[x] for x in nodes if x in graph.pos]
    if k_dist > 0:
        level = graph._g.set_levels([0, len(seeds)], seeds, int(k_dist))[0]
    else:
        level = np.full(len(graph.names), -1, dtype=np.int32)
    return _k_path_from_rings(_rings_from_levels(level, graph.selfloop, graph.names, graph.pos, nodes, k_dist), full_trail,
                              trail_start)


def get_k_path_neighbours(mapping_h5_fn, ref_name, nodes, k_dist, full_trail=False, trail_start=0, device=0):
    """Graph.get_k_path_neighbours from the mapping file; see RefGraph.k_path_neighbours."""
    with RefGraph(mapping_h5_fn, ref_name, device) as g:
        return g.k_path_neighbours(nodes, k_dist, full_trail, trail_start)


# ---- Test / Control / Other ---------------------------------------------------------------------------------------
def _valid_nodes(ref_nodes, from_clusters, cluster_dict):
    """the reference nodes Test cells may come from (:1016-1028): the checks, then the cluster filter"""
    if from_clusters is None:
        return list(ref_nodes)
    _validate_clusters(cluster_dict)
    if type(from_clusters) != list:
        raise TypeError("ERROR: from_cluster parameter value should be a list")
    from_clusters = {str(x): None for x in from_clusters}
    return [i for i in ref_nodes if i in cluster_dict and cluster_dict[i] in from_clusters]


def _de_groups(ref_nodes, valid_nodes, valid_scores, k_path, node_dist, full_trail, trail_start, stringent_control):
    """set_de_groups (:1029-1052) after the cluster filter and the mapping scores; k_path(nodes, k_dist, full_trail,
    trail_start) -> names"""
    test_nodes = {x: None for x in valid_nodes if x in valid_scores}
    if len(test_nodes) < 5:
        print('WARNING: Less than 5 test nodes found! Will not set "de_group"')
        return None
    control_nodes = k_path(list(test_nodes.keys()), node_dist, full_trail, trail_start)
    if stringent_control:
        control_nodes = {x: None for x in control_nodes if x not in valid_scores}
    else:
        control_nodes = {x: None for x in control_nodes}
    de_group = {n: "Test" if n in test_nodes else "Control" if n in control_nodes else "Other" for n in ref_nodes}
    test_cells = [x.rsplit("_", 1)[0] for x in test_nodes]
    ctrl_cells = [x.rsplit("_", 1)[0] for x in control_nodes]
    print("Test nodes: %d, Control nodes: %d" % (len(test_cells), len(ctrl_cells)), flush=True)
    return {"de_group": de_group, "deTestCells": test_cells, "deCtrlCells": ctrl_cells}


def _set_de_groups(graph, target, min_score, node_dist, from_clusters, full_trail, trail_start, stringent_control, clusters):
    from ._score import get_mapping_score
    # as the reference: the clusters and the type of from_clusters are checked before anything is scored
    valid_nodes = _valid_nodes(graph.ref_nodes, from_clusters,
                               _imported_clusters(graph.ref_nodes, clusters) if from_clusters is not None else {})
    valid_scores = get_mapping_score(graph.fn, graph.ref_name, target, min_score=min_score, all_nodes=False)
    return _de_groups(graph.ref_nodes, valid_nodes, valid_scores, lambda *a: _k_path_neighbours(graph, *a), node_dist, full_trail,
                      trail_start, stringent_control)


def get_de_groups(mapping_h5_fn, ref_name, target, min_score, node_dist, from_clusters=None, full_trail=False, trail_start=1,
                  stringent_control=False, clusters=None, device=0):
    """Graph.set_de_groups from the mapping file, returning what the reference stores on the Graph object; see
    RefGraph.set_de_groups."""
    with RefGraph(mapping_h5_fn, ref_name, device) as g:
        return g.set_de_groups(target, min_score, node_dist, from_clusters, full_trail, trail_start, stringent_control, clusters)


# ---- mapped cells (host only) -------------------------------------------------------------------------------------
def _mapped_cells(pos, ref_name, t_nodes, ptr, nbr, ref_cells, remove_suffix):
    want = set()
    for i in ref_cells:
        if remove_suffix:
            i = i + "_" + ref_name
        if i in pos:
            want.add(pos[i])
    hit = np.isin(np.asarray(nbr), np.fromiter(want, dtype=np.int64, count=len(want)))
    rows = np.unique(np.repeat(np.arange(len(t_nodes)), np.diff(ptr))[hit])
    mapped = [t_nodes[i] for i in rows.tolist()]
    return sorted(x.rsplit("_", 1)[0] for x in mapped) if remove_suffix else sorted(mapped)


def get_mapped_cells(mapping_h5_fn, ref_name, target, ref_cells, remove_suffix=True):
    """Graph.get_mapped_cells (nabo/_graph.py:859-884): the target cells of sample `target` connected to any of the
    reference cells `ref_cells` (cell names; NODE names `<cell>_<ref_name>` when remove_suffix is False, and then node
    names are returned).  Reference cells the graph does not know are ignored; an unknown target raises ValueError
    (:870-871).  The reference returns list(set(...)), an arbitrary order: here the returned list is sorted.  Host code:
    no GPU is used."""
    import h5py
    with h5py.File(mapping_h5_fn, "r") as h5:
        _, pos, _ = _open_ref(h5, ref_name)
        try:
            t_nodes, ptr, nbr, _ = _target_rows_w(h5, target, pos)
        except KeyError:
            raise ValueError("ERROR: %s not present in graph!" % target)
    return _mapped_cells(pos, ref_name, t_nodes, ptr, nbr, ref_cells, remove_suffix)
