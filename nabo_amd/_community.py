"""Clusters of the reference graph on the GPU: seeded synchronous Louvain on exact integers, and the modularity of any
labelling.

Array / HDF5 restatement of `Graph.make_leiden_clusters` (nabo/_graph.py:266-292), `Graph.calc_modularity` (:415-442)
and the two cluster writers (`save_clusters_as_json`, `save_clusters_as_csv`, :387-402).  The reference hands `refG` to
leidenalg + igraph; here `nabo_community_run` (include/nabo_community.h, nabo_amd/csrc/community.hip) runs on the
device.  include/nabo_community.h holds the definition; leidenalg's own partitions and random stream are not pinned
(DESIGN.md 4.15).

`Graph.make_clusters` (:247-264, Newman's greedy agglomeration through `hac`) is here too: `nabo_community_agglomerate`
(include/nabo_agglom.h, nabo_amd/csrc/agglom.hip) merges a greedy matching of the best cluster pairs per round on the same
handle and the same integers, keeps the dendrogram, and `nabo_community_cut` reads any number of clusters off it
(DESIGN.md 4.18); hac's own merge order is not pinned.
"""
import ctypes as C
import json

import numpy as np

from . import _lib
from ._graphio import Handle, check_csr as _check_graph, read_ref_graph as _ref_graph_csr

PHASES = ("sweeps", "aggregate", "finish", "run")
AGGLOM_PHASES = ("passes", "order", "aggregate", "run")


def geometry():
    """(group, long_threshold, table_capacity) of the sweep as built: `group` lanes share a row of at most
    `long_threshold` arcs, a longer row takes a workgroup whose LDS table holds `table_capacity` distinct neighbour
    communities, a row with more a table in global memory; needs no device"""
    a, b, c = C.c_int32(), C.c_int32(), C.c_int32()
    _lib.check(_lib.lib().nabo_community_geometry(C.byref(a), C.byref(b), C.byref(c)))
    return int(a.value), int(b.value), int(c.value)


def quantise(w, weight_scale=10000):
    """q = rint(w * weight_scale) as int64: the integer weights every sum of the clustering is taken in"""
    return np.rint(np.asarray(w, dtype=np.float64) * float(weight_scale)).astype(np.int64)


def _int(v, name, lo, hi=None):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
        raise ValueError("ERROR: %s must be an integer" % name)
    if v < lo or (hi is not None and v > hi):
        raise ValueError("ERROR: %s=%d must be %s" % (name, v, "at least %d" % lo if hi is None else "in [%d, %d]" % (lo, hi)))
    return int(v)


def _check_params(resolution, seed, weight_scale, max_sweeps, max_levels):
    try:
        resolution, weight_scale = float(resolution), float(weight_scale)
    except (TypeError, ValueError):
        raise ValueError("ERROR: resolution and weight_scale must be numbers")
    if not np.isfinite(resolution) or resolution < 0:
        raise ValueError("ERROR: resolution must be finite and not negative")
    if not np.isfinite(weight_scale) or weight_scale <= 0:
        raise ValueError("ERROR: weight_scale must be finite and positive")
    return (resolution, _int(seed, "seed", 0, 2 ** 64 - 1), weight_scale, _int(max_sweeps, "max_sweeps", 1, 2 ** 31 - 1),
            _int(max_levels, "max_levels", 1, 2 ** 31 - 1))


def _check_weights(w, weight_scale):
    if w.size and w.min() < 0:
        raise ValueError("ERROR: w holds a negative weight")
    if w.size and float(np.rint(w.max() * weight_scale)) > 2.0 ** 31:
        raise ValueError("ERROR: the largest weight quantises above 2^31: lower weight_scale")


def _labels(labels, n):
    try:
        lab = np.asarray(labels)
        if lab.dtype.kind not in "iu":
            raise TypeError
        lab = np.ascontiguousarray(lab, dtype=np.int64)
    except (TypeError, ValueError):
        raise ValueError("ERROR: labels must be integers")
    if lab.ndim != 1 or lab.shape[0] != n:
        raise ValueError("ERROR: labels must be 1-D with %d entries" % n)
    if lab.size and (lab.min() < -2 ** 31 or lab.max() >= 2 ** 31):
        raise ValueError("ERROR: labels must fit 32 bits")
    return np.ascontiguousarray(lab, dtype=np.int32)


class Community(Handle):
    """A graph resident on one device and the state of its clustering (nabo_community_create): the handle the tests and
    tools/bench_community.py step through; `louvain_csr` and `modularity_csr` are the one-call forms.  The agglomeration
    (`agglomerate`, `dendrogram`, `cut`; `agglomerate_csr` is its one-call form) runs on the same handle."""
    _destroy = "nabo_community_destroy"

    def __init__(self, ptr, nbr, w, resolution=1.0, seed=4466, weight_scale=10000, max_sweeps=128, max_levels=32, split=True,
                 device=0):
        self.n, ptr, nbr, w = _check_graph(ptr, nbr, w)
        p = _check_params(resolution, seed, weight_scale, max_sweeps, max_levels)
        _check_weights(w, p[2])
        h = C.c_void_p()
        _lib.check(_lib.lib().nabo_community_create(C.byref(h), int(device), int(self.n), ptr.ctypes.data, nbr.ctypes.data, w.ctypes.data, p[2]))
        self._h = h
        self.weight_scale = p[2]
        self.set_params(resolution, seed, max_sweeps, max_levels, split)

    def set_params(self, resolution=1.0, seed=4466, max_sweeps=128, max_levels=32, split=True):
        p = _check_params(resolution, seed, self.weight_scale, max_sweeps, max_levels)
        _lib.check(_lib.lib().nabo_community_set_params(self._h, p[0], p[1], p[3], p[4], int(bool(split))))
        self.resolution = p[0]

    def run(self):
        """the whole run; (labels int32 [n] in 1 .. C, info) as louvain_csr returns them"""
        L = _lib.lib()
        _lib.check(L.nabo_community_run(self._h))
        labels = np.empty(self.n, dtype=np.int32)
        nc, q, nr = C.c_int32(), C.c_double(), C.c_int64()
        _lib.check(L.nabo_community_labels(self._h, labels.ctypes.data, C.byref(nc), C.byref(q)))
        _lib.check(L.nabo_community_history(self._h, C.byref(nr), 0, None, None))
        rec, hq = np.zeros((max(nr.value, 1), 4), dtype=np.int64), np.zeros(max(nr.value, 1), dtype=np.float64)
        _lib.check(L.nabo_community_history(self._h, C.byref(nr), int(nr.value), rec.ctypes.data, hq.ctypes.data))
        history = [(int(r[0]), int(r[1]), int(r[2]), int(r[3]), float(x)) for r, x in zip(rec[:nr.value], hq[:nr.value])]
        return labels, {"q": q.value, "n_clusters": int(nc.value), "two_m": self.level_size()[2], "history": history, "ms": self.last_ms()}

    def modularity(self, labels, resolution=None):
        """the modularity of any labelling of the level-0 nodes (equal value = same cluster)"""
        lab = _labels(labels, self.n)
        q = C.c_double()
        _lib.check(_lib.lib().nabo_community_modularity(self._h, lab.ctypes.data, float(self.resolution if resolution is None else resolution),
                                                        C.byref(q)))
        return q.value

    def split(self, labels, split=True):
        """the result step alone: (labels 1 .. C by size, C), every cluster replaced by its connected components if split"""
        lab = _labels(labels, self.n)
        out, nc = np.empty(self.n, dtype=np.int32), C.c_int32()
        _lib.check(_lib.lib().nabo_community_split(self._h, lab.ctypes.data, int(bool(split)), out.ctypes.data, C.byref(nc)))
        return out, int(nc.value)

    def level_size(self):
        """(n, n_arcs, two_m) of the current level"""
        a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
        _lib.check(_lib.lib().nabo_community_level_size(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return int(a.value), int(b.value), int(c.value)

    def get_level(self):
        """{"ptr", "nbr", "a", "k", "in": int64} of the current level"""
        n, A, _ = self.level_size()
        ptr, nbr, a = np.zeros(n + 1, dtype=np.int64), np.zeros(A, dtype=np.int64), np.zeros(A, dtype=np.int64)
        k, inn = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
        _lib.check(_lib.lib().nabo_community_get_level(self._h, ptr.ctypes.data, nbr.ctypes.data, a.ctypes.data, k.ctypes.data, inn.ctypes.data))
        return {"ptr": ptr, "nbr": nbr, "a": a, "k": k, "in": inn}

    def set_comm(self, comm):
        n = self.level_size()[0]
        comm = _labels(comm, n)
        if comm.size and (comm.min() < 0 or comm.max() >= n):
            raise ValueError("ERROR: comm holds an entry that is not a community in [0, %d)" % n)
        _lib.check(_lib.lib().nabo_community_set_comm(self._h, comm.ctypes.data))

    def get_comm(self):
        comm = np.empty(self.level_size()[0], dtype=np.int32)
        _lib.check(_lib.lib().nabo_community_get_comm(self._h, comm.ctypes.data))
        return comm

    def sweep(self, level, sweep):
        """one sweep of the current level from the current comm: (moved, want)"""
        mv, want = C.c_int64(), C.c_int64()
        _lib.check(_lib.lib().nabo_community_sweep(self._h, int(level), int(sweep), C.byref(mv), C.byref(want)))
        return int(mv.value), int(want.value)

    def aggregate(self):
        _lib.check(_lib.lib().nabo_community_aggregate(self._h))

    def rewind(self):
        _lib.check(_lib.lib().nabo_community_rewind(self._h))

    def last_ms(self):
        """{"sweeps", "aggregate", "finish", "run": device ms of the last run}"""
        ms = (C.c_double * 4)()
        _lib.check(_lib.lib().nabo_community_last_ms(self._h, ms))
        return dict(zip(PHASES, ms[:4]))

    # ---- greedy modularity agglomeration (include/nabo_agglom.h) ----
    def agglomerate(self, n_min=1):
        """the whole agglomeration from level 0 until `n_min` clusters are left or no arc is; the info of agglomerate_csr
        without "q" and "n_clusters", which belong to a cut"""
        _lib.check(_lib.lib().nabo_community_agglomerate(self._h, _int(n_min, "n_min", 1, self.n)))
        info = (C.c_int64 * 4)()
        _lib.check(_lib.lib().nabo_community_agglom_info(self._h, info))
        rec, q_path = self.dendrogram()
        return {"rounds": int(info[0]), "passes": int(info[1]), "peak": int(info[2]), "n_end": int(info[3]), "merges": rec, "q_path": q_path,
                "two_m": self.level_size()[2], "ms": self.agglom_ms()}

    def dendrogram(self):
        """(merges int64 [M, 6]: rep_a < rep_b, round, a_cd, k_a, k_b per merge in order; q_path float64 [M + 1]: the
        modularity after 0 .. M merges) of the last agglomeration"""
        L, nm = _lib.lib(), C.c_int64()
        _lib.check(L.nabo_community_dendrogram(self._h, C.byref(nm), 0, None, None))
        rec, q_path = np.zeros((nm.value, 6), dtype=np.int64), np.zeros(nm.value + 1, dtype=np.float64)
        _lib.check(L.nabo_community_dendrogram(self._h, C.byref(nm), int(nm.value), rec.ctypes.data, q_path.ctypes.data))
        return rec, q_path

    def cut(self, n_clusters=0):
        """(labels int32 [n] in 1 .. C by descending size, C, Q) after the first n - n_clusters merges of the last
        agglomeration; n_clusters = 0: at the peak of Q.  ValueError outside [the clusters at the run's end, n]."""
        labels, nc, q = np.empty(self.n, dtype=np.int32), C.c_int32(), C.c_double()
        _lib.check(_lib.lib().nabo_community_cut(self._h, _int(n_clusters, "n_clusters", 0), labels.ctypes.data, C.byref(nc), C.byref(q)))
        return labels, int(nc.value), q.value

    def match_pass(self, free=None):
        """one locally dominant pass on the current level: (partner int32 [n], -1 for none; D, the winning gains as Python
        integers, 0 for none).  free: [n], false = the cluster takes no part (None: all are free)."""
        n = self.level_size()[0]
        f = None
        if free is not None:
            f = np.ascontiguousarray(np.asarray(free).astype(bool), dtype=np.uint8)
            if f.shape != (n,):
                raise ValueError("ERROR: free must be 1-D with %d entries" % n)
        partner, hi, lo = np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int64), np.empty(n, dtype=np.uint64)
        _lib.check(_lib.lib().nabo_community_match_pass(self._h, None if f is None else f.ctypes.data, partner.ctypes.data, hi.ctypes.data,
                                                        lo.ctypes.data))
        return partner, [(h << 64) + x for h, x in zip(hi.tolist(), lo.tolist())]

    def match(self):
        """one round's matching on the current level: (pairs int32 [m, 2], c < d, in pair order; passes).  comm is left set
        for them, so that aggregate() follows."""
        n = self.level_size()[0]
        pairs, m, p = np.zeros((n // 2 + 1, 2), dtype=np.int32), C.c_int64(), C.c_int64()
        _lib.check(_lib.lib().nabo_community_match(self._h, C.byref(m), C.byref(p), pairs.ctypes.data))
        return pairs[:m.value].copy(), int(p.value)

    def agglom_ms(self):
        """{"passes", "order", "aggregate", "run": device ms of the last agglomeration}"""
        ms = (C.c_double * 4)()
        _lib.check(_lib.lib().nabo_community_agglom_ms(self._h, ms))
        return dict(zip(AGGLOM_PHASES, ms[:4]))


def louvain_csr(ptr, nbr, w, resolution=1.0, seed=4466, weight_scale=10000, max_sweeps=128, max_levels=32, split=True, device=0):
    """Clusters of the weighted graph a CSR (ptr, nbr, w) describes -- rows in either arc direction; a pair listed more
    than once keeps its last weight, self-loops are kept -- by the seeded synchronous Louvain of include/nabo_community.h.
    Returns (labels int32 [n] in 1 .. C by descending size, info): info["q"] the modularity of the labels at
    `resolution`, "n_clusters", "two_m" (the quantised 2m), "history" [(n, n', sweeps, moved, Q) per level] and "ms".
    Weights are quantised to integers, q = rint(w * weight_scale); the same call gives the same labels every time."""
    with Community(ptr, nbr, w, resolution, seed, weight_scale, max_sweeps, max_levels, split, device) as H:
        return H.run()


def modularity_csr(ptr, nbr, w, labels, resolution=1.0, weight_scale=10000, device=0):
    """The modularity of `labels` (any integers, equal value = same cluster) on the graph of louvain_csr, from exact
    integer sums: sum_c in_c / 2m - resolution * sum_c d_c^2 / (2m)^2.  With resolution = 1 this is the quantity
    Graph.calc_modularity computes in floats."""
    n = _check_graph(ptr, nbr, w)[0]
    labels = _labels(labels, n)
    with Community(ptr, nbr, w, resolution, 0, weight_scale, device=device) as H:
        return H.modularity(labels)


def _leiden_of_graph(ref_nodes, pos, ptr, nbr, w, resolution, random_seed, device):
    labels, info = louvain_csr(ptr, nbr, w, resolution=resolution, seed=random_seed, device=device)
    return {x: str(int(labels[pos[x]])) for x in ref_nodes}, info


def make_leiden_clusters(mapping_h5_fn, ref_name, resolution=1.0, random_seed=4466, device=0):
    """Graph.make_leiden_clusters (nabo/_graph.py:266-292) from the mapping file: {reference node: str(cluster)} in the
    reference's node order (`refNodes`, the file's), clusters numbered from 1 by descending size as leidenalg numbers
    them.  The dict is what classify_target(cluster_dict=...) and get_de_groups(..., clusters=...) take.

    What differs from the reference, which calls leidenalg.find_partition with RBConfigurationVertexPartition
    (DESIGN.md 4.15): the moves are Louvain's (synchronous sweeps, seeded gate), followed by a split of every cluster
    into its connected components in place of Leiden's refinement, so clusters are connected but leidenalg's partition is
    not reproduced; the objective is the same (RB configuration model at `resolution`); the result is deterministic --
    the same call gives the same clusters, bit for bit; and the weights are quantised to integers
    (rint(w * 10000): Nabo's hundredths are exact)."""
    ref_nodes, pos, _, ptr, nbr, w = _ref_graph_csr(mapping_h5_fn, ref_name)
    return _leiden_of_graph(ref_nodes, pos, ptr, nbr, w, resolution, random_seed, device)[0]


def agglomerate_csr(ptr, nbr, w, n_clusters=None, weight_scale=10000, device=0):
    """Clusters of the weighted graph of louvain_csr by the greedy modularity agglomeration of include/nabo_agglom.h:
    every round merges a greedy matching of the cluster pairs whose merge raises the modularity most, until one cluster
    per connected component is left; `n_clusters` are then read off the merge list (None: at the peak of Q).  Returns
    (labels int32 [n] in 1 .. C by descending size, info): info["q"] the modularity of the labels at resolution 1,
    "n_clusters", "rounds", "passes", "merges" (int64 [M, 6]: rep_a < rep_b, round, a_cd, k_a, k_b), "q_path" (the
    modularity after 0 .. M merges), "peak" (the number of merges at the largest Q), "n_end", "two_m" and "ms".
    ValueError if n_clusters is below the clusters at the run's end or above the node count.  Every sum is an integer
    one: the same call gives the same labels every time."""
    if n_clusters is not None:
        n_clusters = _int(n_clusters, "n_clusters", 1)
    with Community(ptr, nbr, w, 1.0, 0, weight_scale, device=device) as H:
        info = H.agglomerate()
        labels, info["n_clusters"], info["q"] = H.cut(0 if n_clusters is None else n_clusters)
        return labels, info


def _clusters_of_graph(ref_nodes, pos, H, n_clusters):
    """the dict of make_clusters from a handle whose agglomeration has run"""
    labels = H.cut(_int(n_clusters, "n_clusters", 1))[0]
    return {x: str(int(labels[pos[x]])) for x in ref_nodes}


def make_clusters(mapping_h5_fn, ref_name, n_clusters, device=0):
    """Graph.make_clusters (nabo/_graph.py:247-264) from the mapping file: {reference node: str(cluster)} in the
    reference's node order with exactly `n_clusters` clusters, numbered from 1 by descending size; the dict of
    make_leiden_clusters.  ValueError if `n_clusters` is below the number of clusters at the run's end (one per connected
    component of the graph) or above the node count.

    What differs from the reference, which hands `refG` to hac.GreedyAgglomerativeClusterer: a round
    merges a whole greedy matching of the best pairs where Newman's algorithm merges one pair, so hac's merge order is
    not reproduced; the objective, the gain of a merge and the rule `best first` are the same; the weights are quantised
    to integers (rint(w * 10000): Nabo's hundredths are exact) and the result is the same bit for bit on every call."""
    ref_nodes, pos, _, ptr, nbr, w = _ref_graph_csr(mapping_h5_fn, ref_name)
    with Community(ptr, nbr, w, device=device) as H:
        H.agglomerate()
        return _clusters_of_graph(ref_nodes, pos, H, n_clusters)


def _modularity_of_graph(ref_nodes, pos, ptr, nbr, w, clusters, device):
    if sum(1 for x in ref_nodes if x in clusters) != len(ref_nodes) or len(clusters) != len(ref_nodes):
        raise AssertionError("ERROR: Not all reference nodes have been assigned to a cluster. Cannot calculate modularity!")
    ids = {}
    labels = np.zeros(len(ptr) - 1, dtype=np.int32)
    labels[:] = -1 - np.arange(len(labels))                  # a node of the file that is not in refNodes stands alone
    for x in ref_nodes:
        labels[pos[x]] = ids.setdefault(clusters[x], len(ids))
    return modularity_csr(ptr, nbr, w, labels, 1.0, device=device)


def calc_modularity(mapping_h5_fn, ref_name, clusters, device=0):
    """Graph.calc_modularity (nabo/_graph.py:415-442): the modularity of the reference graph under `clusters`
    ({reference node: cluster}, as make_leiden_clusters returns or Graph.import_clusters takes), from exact integer sums
    of the quantised weights where the reference adds floats.  AssertionError, with the reference's text, unless every
    reference node has a cluster."""
    ref_nodes, pos, _, ptr, nbr, w = _ref_graph_csr(mapping_h5_fn, ref_name)
    return _modularity_of_graph(ref_nodes, pos, ptr, nbr, w, clusters, device)


def save_clusters_as_json(clusters, out_fn):
    """Graph.save_clusters_as_json (nabo/_graph.py:387-394): what Graph.import_clusters_from_json reads"""
    with open(out_fn, "w") as out:
        json.dump({k: str(v) for k, v in clusters.items()}, out, indent=2)


def save_clusters_as_csv(clusters, out_fn):
    """Graph.save_clusters_as_csv (nabo/_graph.py:396-402; `pd.Series(self.clusters).to_csv(outfn)`): a header line
    `,0`, then one line `node,cluster` per node."""
    with open(out_fn, "w") as out:
        out.write(",0\n")
        for k, v in clusters.items():
            k = str(k)
            if any(c in k for c in ',"\n\r'):
                k = '"' + k.replace('"', '""') + '"'
            out.write("%s,%s\n" % (k, v))
