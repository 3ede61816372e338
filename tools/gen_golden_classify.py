#!/opt/conda/bin/python3.9
"""Golden vectors for the classification and DE-group methods of the reference's Graph (nabo/_graph.py):
classify_target (:722-792), get_k_path_neighbours (:956-987), set_de_groups (:989-1055), get_mapped_cells (:859-884).

TEST INFRASTRUCTURE ONLY, run where the reference is mounted, with an interpreter that has networkx and pandas:

    /opt/conda/bin/python3.9 tools/gen_golden_classify.py

The reference's nabo/_graph.py is loaded BY FILE PATH (as tools/gen_golden_paths.py does).  Its Graph is rebuilt from
the edge lists stored in tests/golden/mapping_small.npz (targets ME, IG) and c1_3k.npz (target ME), nodes and rows
added in the order Graph.load_from_h5 would add them (nabo/_graph.py:93-107), WITH the stored weights.  The graphs'
structure is the one tests/golden/paths.npz already holds (checked here); this file adds the target edges' weights,
the clusters (written by this script: nearest of 8 seeded nodes by BFS) and the reference's results.  Only DATA is
written, to tests/golden/classify.npz.
"""
import io
import json
import os
import sys
from contextlib import redirect_stdout

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from gen_golden_paths import GOLD, call, csr, load_graph_module, rows_of  # noqa: E402

# (weight_frac, min_weight, min_degree).  The generator asserts that deciding ties (two clusters sharing the best weight
# above the threshold, where the reference's pick follows string hashing) are at most 1 % of a case's nodes and absent at
# weight_frac >= 0.5.  SNN weights are quantised, so on mapping_small weight_frac 0.3 and 0.4 give 2 % such nodes: the
# cases below one half use 0.45 and 0.48.  min_weight 0 at weight_frac exactly 0.5 gives ties by rounding of the total
# (two clusters of s each, total a hair under 2s): that case uses 0.6.
CLASSIFY_GRID = [(0.5, 0.1, 2), (0.6, 0.0, 2), (0.45, 0.1, 2), (0.48, 0.06, 1), (0.5, 0.1, 8), (0.7, 0.2, 3)]


def load_graph(gr, ref_name, ref_rows, targets):
    """Graph.load_from_h5 without the file; rows are {node: [(neighbour, weight), ...]}"""
    g = gr.Graph()
    for node, row in ref_rows.items():
        g.add_node(node, kind="reference", name=ref_name)
        for j, w in row:
            g.add_edge(node, j, weight=w)
    g.refName = ref_name
    g.refNodes = list(ref_rows)
    g.refG = g.subgraph(g.refNodes)
    for tname, trows in targets.items():
        for node, row in trows.items():
            g.add_node(node, kind="target", name=tname)
            for j, w in row:
                g.add_edge(node, j, weight=w)
        g.targetNames.append(tname)
        g.targetNodes[tname] = list(trows)
    return g


def rows_w(nodes, src, dst, w):
    rows = {n: [] for n in nodes}
    for s, d, x in zip(src.tolist(), dst.tolist(), w.tolist()):
        rows[s].append((d, x))
    return rows


def bfs_clusters(n, ptr, nbr, n_seeds, seed):
    """cluster of every node = index of the nearest of n_seeds seeded nodes (BFS over both arc directions, lowest
    seed index first); unreachable nodes go to cluster 0"""
    adj = [[] for _ in range(n)]
    for u in range(n):
        for v in nbr[ptr[u]:ptr[u + 1]].tolist():
            adj[u].append(v)
            adj[v].append(u)
    rng = np.random.default_rng(seed)
    seeds = rng.choice(n, n_seeds, replace=False).tolist()
    lab = np.full(n, -1, dtype=np.int64)
    front = []
    for i, s in enumerate(seeds):
        lab[s] = i
        front.append(s)
    while front:
        nxt = []
        for u in front:
            for v in adj[u]:
                if lab[v] < 0:
                    lab[v] = lab[u]
                    nxt.append(v)
        front = nxt
    lab[lab < 0] = 0
    return lab + 1                  # cluster numbers start from 1, as import_clusters' docstring asks


def quiet(fn, *a, **k):
    with redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def deciding_ties(g, target, cluster_dict, weight_frac, min_degree, min_weight):
    """indices of the target nodes whose best cluster weight is shared by two or more clusters AND passes the
    threshold: the label then depends on which of them max() meets first.  From the sums, not from the pick."""
    out = []
    deg = dict(g.degree)
    clusts = set(cluster_dict.values())
    for idx, i in enumerate(g.targetNodes[target]):
        if deg[i] < min_degree:
            continue
        cw = {x: 0 for x in clusts}
        tot = 0
        for j in g.edges(i, data=True):
            if j[2]["weight"] > min_weight and j[1] in cluster_dict:
                cw[cluster_dict[j[1]]] += j[2]["weight"]
            tot += j[2]["weight"]
        top = max(cw.values())
        if top > weight_frac * tot and sum(1 for v in cw.values() if v == top) > 1:
            out.append(idx)
    return out


def classify_cases(g, tag, t, ref_nodes, variants, out, cases):
    n_t = len(g.targetNodes[t])
    for vname, named in variants.items():
        for form in ("clusters", "cluster_dict"):
            if form == "clusters":
                quiet(g.import_clusters, named)
                effective = dict(g.clusters)
            else:
                effective = dict(named)
            for wf, mw, md in CLASSIFY_GRID:
                key = "%s_%s_%s_%s_%g_%g_%d" % (tag, t, vname, form, wf, mw, md)
                kw = dict(weight_frac=wf, min_weight=mw, min_degree=md)
                if form == "cluster_dict":
                    kw.update(cluster_dict=named, na_label="unk")
                res = g.classify_target(t, **kw)
                cnt = g.classify_target(t, ret_counts=True, **kw)
                assert list(res) == list(g.targetNodes[t])
                tied = deciding_ties(g, t, effective, wf, md, mw)
                assert len(tied) <= 0.01 * n_t, (key, len(tied), n_t)
                assert wf < 0.5 or not tied, (key, tied)
                out[key + "_labels"] = np.array([str(v) for v in res.values()])
                out[key + "_tied"] = np.array(tied, dtype=np.int32)
                cases.append({"key": key, "tag": tag, "target": t, "variant": vname, "form": form, "weight_frac": wf,
                              "min_weight": mw, "min_degree": md, "counts": {str(k): int(v) for k, v in cnt.items()}})
                print("  %s: %d tied, %d unclassified" % (key, len(tied), sum(1 for v in res.values() if v in ("NA", "unk"))))


def fixture_cases(gr, out):
    specs = [("small", "mapping_small.npz", ["ME", "IG"]), ("c1", "c1_3k.npz", ["ME"])]
    paths = np.load(os.path.join(GOLD, "paths.npz"))
    cases, rings, groups, mapped = [], [], [], []
    for tag, fn, tnames in specs:
        d = np.load(os.path.join(GOLD, fn))
        ref_nodes = [str(x) for x in d["ref_graph_nodes"]]
        ref_rows = rows_w(ref_nodes, d["ref_graph_src"], d["ref_graph_dst"], d["ref_graph_w"])
        index = {n: i for i, n in enumerate(ref_nodes)}
        t_rows = {t: rows_w([str(x) for x in d["t_%s_graph_nodes" % t]], d["t_%s_graph_src" % t], d["t_%s_graph_dst" % t],
                            d["t_%s_graph_w" % t]) for t in tnames}
        g = load_graph(gr, "WT", ref_rows, t_rows)
        # the structure is the one paths.npz holds: only weights, clusters and results are added here
        assert ref_nodes == [str(x) for x in paths[tag + "_ref_nodes"]]
        ptr, nbr = csr({n: [j for j, _ in r] for n, r in ref_rows.items()}, index)
        assert np.array_equal(ptr, paths[tag + "_ref_ptr"]) and np.array_equal(nbr, paths[tag + "_ref_nbr"])
        lab = bfs_clusters(len(ref_nodes), ptr, nbr, 8, seed=17)
        unnamed = np.zeros(len(ref_nodes), dtype=bool)
        unnamed[np.random.default_rng(23).choice(len(ref_nodes), len(ref_nodes) // 10, replace=False)] = True
        out[tag + "_clusters"] = lab.astype(np.int32)
        out[tag + "_unnamed"] = unnamed
        variants = {"full": {n: int(lab[i]) for i, n in enumerate(ref_nodes)},
                    "partial": {n: int(lab[i]) for i, n in enumerate(ref_nodes) if not unnamed[i]}}
        for t in tnames:
            p = "%s_%s" % (tag, t)
            tp, tn = csr({n: [j for j, _ in r] for n, r in t_rows[t].items()}, index)
            assert np.array_equal(tp, paths[p + "_t_ptr"]) and np.array_equal(tn, paths[p + "_t_nbr"])
            assert list(t_rows[t]) == [str(x) for x in paths[p + "_t_nodes"]]
            out[p + "_t_w"] = np.array([w for r in t_rows[t].values() for _, w in r], dtype=np.float64)
            classify_cases(g, tag, t, ref_nodes, variants, out, cases)
            # rings around the top-scoring reference nodes
            top = g.get_mapping_score(t, sorted_names_only=True)[:30]
            for k in range(5):
                for full, start in ((False, 0), (True, 0), (True, 1), (True, k), (True, k + 2)):
                    res = g.get_k_path_neighbours(top, k, full_trail=full, trail_start=start)
                    pos = [index[x] for x in res]
                    rings.append({"tag": tag, "target": t, "nodes": [index[x] for x in top], "k_dist": k, "full_trail": full,
                                  "trail_start": start, "as_given": k == 0 and not full,
                                  "result": pos if (k == 0 and not full) else sorted(pos)})
            # Test / Control / Other
            quiet(g.import_clusters, variants["full"])
            scores = np.array(list(g.get_mapping_score(t).values()))
            cut = float(np.percentile(scores, 90))
            top_clusters = [int(c) for c in np.unique(lab[np.nonzero(scores >= cut)[0]])[:3]]
            for kw in ({"min_score": cut, "node_dist": 2},
                       {"min_score": cut, "node_dist": 3, "full_trail": True},
                       {"min_score": cut, "node_dist": 3, "full_trail": True, "trail_start": 2, "stringent_control": True},
                       {"min_score": cut, "node_dist": 1, "stringent_control": True},
                       {"min_score": cut, "node_dist": 2, "from_clusters": top_clusters},
                       {"min_score": cut, "node_dist": 2, "from_clusters": top_clusters, "full_trail": True, "stringent_control": True},
                       {"min_score": float(scores.max()) + 1.0, "node_dist": 2}):
                g.deTestCells, g.deCtrlCells = None, None
                for n in g.refNodes:
                    g.nodes[n].pop("de_group", None)
                quiet(g.set_de_groups, t, **kw)
                if g.deTestCells is None:
                    res = None
                else:
                    code = {"Other": 0, "Test": 1, "Control": 2}
                    res = {"de_group": [code[g.nodes[n]["de_group"]] for n in g.refNodes], "deTestCells": list(g.deTestCells),
                           "deCtrlCells": sorted(g.deCtrlCells)}
                    assert len(g.deTestCells) >= 5
                groups.append({"tag": tag, "target": t, "kwargs": kw, "result": res})
            assert sum(1 for x in groups if x["tag"] == tag and x["target"] == t and x["result"] is None) == 1
            # mapped cells
            cells = [n.rsplit("_", 1)[0] for n in ref_nodes]
            for lst, rs in (([cells[0]], True), (cells[3:40], True), ([ref_nodes[5], ref_nodes[77]], False),
                            (cells[:5] + ["no_such_cell"], True), ([], True), (cells[:3], False)):
                mapped.append({"tag": tag, "target": t, "ref_cells": lst, "remove_suffix": rs,
                               "result": sorted(g.get_mapped_cells(t, lst, remove_suffix=rs))})
    out["cases"] = np.array(json.dumps(cases))
    out["rings"] = np.array(json.dumps(rings))
    out["de_groups"] = np.array(json.dumps(groups))
    out["mapped_cells"] = np.array(json.dumps(mapped))


def quirk_case(gr):
    """a hand-built graph; node lists are in load order"""
    R = ["r%d_R" % i for i in range(10)]
    # path r0-r1-r2-r3-r4 with a self-loop on r1 and on r3, a branch r2-r5-r6, a second component r8-r9, isolated r7
    ref_rows = {R[0]: [(R[1], 1.0)], R[1]: [(R[1], 1.0), (R[2], 1.0)], R[2]: [(R[3], 1.0), (R[5], 1.0)], R[3]: [(R[3], 1.0)],
                R[4]: [(R[3], 1.0)], R[5]: [(R[6], 1.0)], R[6]: [], R[7]: [], R[8]: [(R[9], 1.0)], R[9]: []}
    targets = {
        "T": {
            "t0_T": [(R[0], 0.5), (R[1], 0.5)],                              # best exactly weight_frac * total (0.5 of 1.0)
            "t1_T": [(R[0], 0.25), (R[4], 0.5), (R[0], 0.75)],               # repeated neighbour: one edge, last weight
            "t2_T": [],                                                      # empty row
            "t3_T": [(R[2], 0.9)],                                           # under min_degree = 2
            "t4_T": [(R[7], 0.6), (R[0], 0.3)],                              # r7 has no cluster
            "t5_T": [(R[0], 0.1), (R[4], 0.2), (R[5], 0.05)],                # a weight exactly min_weight
            "t6_T": [(R[0], 0.25), (R[4], 0.25), (R[8], 0.125)],             # two clusters tied, below the threshold at 0.5
            "t7_T": [(R[8], 0.5), (R[9], 0.25), (R[0], 0.125)],
            "t8_T": [(R[1], 0.05), (R[2], 0.05)],                            # every weight below min_weight
        },
        "W": {},
    }
    cd = {R[0]: "a", R[1]: "a", R[2]: "a", R[3]: "b", R[4]: "b", R[5]: "b", R[6]: "b", R[8]: "c", R[9]: "c", "ghost_R": "d"}
    imp = {R[i]: (1 if i < 3 else 2) for i in range(7)}                      # r7..r9 become 'NA'
    g = load_graph(gr, "R", ref_rows, targets)
    calls = []

    def rec(method, fn, **kw):
        calls.append({"method": method, "kwargs": kw, "result": call(quiet, fn, **kw)})

    rec("classify_target", g.classify_target, target="T")                    # no clusters yet: ValueError
    rec("classify_target", g.classify_target, target="T", cluster_dict={})
    rec("classify_target", g.classify_target, target="W", cluster_dict={})
    quiet(g.import_clusters, {R[i]: 1 for i in range(10)})
    rec("classify_target", g.classify_target, target="T", clusters={R[i]: 1 for i in range(10)})      # one cluster
    quiet(g.import_clusters, imp)
    for kw in ({}, {"ret_counts": True}, {"weight_frac": 0.4}, {"min_degree": 1, "min_weight": 0.0}, {"na_label": "none"},
               {"min_degree": 0}, {"min_degree": 1, "weight_frac": 0.0}):
        rec("classify_target", g.classify_target, target="T", clusters=imp, **kw)
        rec("classify_target", g.classify_target, target="T", cluster_dict=cd, **kw)
    rec("classify_target", g.classify_target, target="missing", clusters=imp)
    rec("classify_target", g.classify_target, target="W", clusters=imp)
    rec("classify_target", g.classify_target, target="W", clusters=imp, ret_counts=True)
    node_sets = [[R[0]], [R[1]], [R[1], R[1]], [R[3], R[0]], [R[7]], [R[8]], ["nobody_R", R[2]], ["nobody_R"], [], [R[2], R[5], R[2]],
                 [R[0], R[4], R[9]]]
    for nodes in node_sets:
        for k in (0, 1, 2, 3, 6):
            for full, start in ((False, 0), (True, 0), (True, 1), (True, -1), (True, 7)):
                rec("k_path_neighbours", g.get_k_path_neighbours, nodes=nodes, k_dist=k, full_trail=full, trail_start=start)
    for lst, rs in (([R[0][:-2]], True), ([R[0]], False), ([R[0]], True), (["r4", "r8", "zz"], True), ([], True)):
        rec("mapped_cells", g.get_mapped_cells, target="T", ref_cells=lst, remove_suffix=rs)
    rec("mapped_cells", g.get_mapped_cells, target="missing", ref_cells=["r0"])
    rec("de_groups", g.set_de_groups, target="T", min_score=0, node_dist=1, from_clusters="1")       # TypeError
    return {"imported": imp, "ref_rows": list(ref_rows.items()), "targets": {t: list(r.items()) for t, r in targets.items()}, "calls": calls}


def strip_reference_only(case):
    """classify_target calls were made on the reference WITHOUT `clusters` (imported beforehand); the key stays in the
    record for this build's function.  Results that are dicts / Counters / lists are stored as JSON; ring results as
    sorted lists (the reference's order is a set's)."""
    for c in case["calls"]:
        kind, res = c["result"]
        if kind == "ok" and c["method"] == "k_path_neighbours":
            as_given = c["kwargs"]["k_dist"] == 0 and not c["kwargs"]["full_trail"]
            c["result"] = (kind, list(res) if as_given else sorted(res))
        elif kind == "ok" and c["method"] == "mapped_cells":
            c["result"] = (kind, sorted(res))
        elif kind == "ok" and c["method"] == "classify_target":
            c["result"] = (kind, {str(k): v for k, v in res.items()})
    return case


def main():
    gr = load_graph_module()
    # the reference's classify_target takes no `clusters`: drop it from the call, keep it in the record
    orig = gr.Graph.classify_target

    def classify_target(self, target, clusters=None, **kw):
        return orig(self, target, **kw)
    gr.Graph.classify_target = classify_target
    out = {}
    fixture_cases(gr, out)
    out["quirks"] = np.array(json.dumps(strip_reference_only(quirk_case(gr))))
    fn = os.path.join(GOLD, "classify.npz")
    np.savez_compressed(fn, **out)
    print("wrote %s (%d bytes; paths.npz is %d)" % (fn, os.path.getsize(fn), os.path.getsize(os.path.join(GOLD, "paths.npz"))))


if __name__ == "__main__":
    sys.exit(main())
