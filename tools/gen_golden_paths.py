#!/opt/conda/bin/python3.9
"""Golden vectors for the hop-distance methods of the reference's Graph (nabo/_graph.py): mapping specificity
(:794-824), reference specificity (:826-857) and contiguous shortest-path lengths (:904-916).

TEST INFRASTRUCTURE ONLY, run where the reference is mounted, with an interpreter that has networkx and pandas:

    /opt/conda/bin/python3.9 tools/gen_golden_paths.py

The reference's nabo/_graph.py is loaded BY FILE PATH (as oracle/gen_golden.py does).  Its Graph is rebuilt from
the edge lists already stored in tests/golden/mapping_small.npz (targets ME, IG) and c1_3k.npz (target ME): nodes
and rows are added in the order Graph.load_from_h5 would add them (nabo/_graph.py:93-107).  A few small hand-built
graphs cover the quirks (a NaN first value, self-loops and duplicate / one-way arcs, a disconnected pair, an empty
target).  Only DATA is written, to tests/golden/paths.npz: the graphs as integer CSR rows and the reference's
results.
"""
import importlib.util
import json
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
REF = os.environ.get("NABO_REFERENCE", "/root/reference")
GOLD = os.path.join(REPO, "tests", "golden")


def load_graph_module():
    spec = importlib.util.spec_from_file_location("nabo_ref_graph", os.path.join(REF, "nabo", "_graph.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def rows_of(nodes, src, dst):
    """{node: [neighbour names in row order]} in `nodes` order (rows of a `<uid>_graph` group)"""
    rows = {n: [] for n in nodes}
    for s, d in zip(src.tolist(), dst.tolist()):
        rows[s].append(d)
    return rows


def load_graph(gr, ref_name, ref_rows, targets):
    """Graph.load_from_h5 without the file: reference first, then each target, nodes and rows in the given order"""
    import networkx as nx  # noqa: F401  (the reference's Graph is an nx.Graph)
    g = gr.Graph()
    for node, row in ref_rows.items():
        g.add_node(node, kind="reference", name=ref_name)
        for j in row:
            g.add_edge(node, j, weight=1.0)
    g.refName = ref_name
    g.refNodes = list(ref_rows)
    g.refG = g.subgraph(g.refNodes)
    for tname, trows in targets.items():
        for node, row in trows.items():
            g.add_node(node, kind="target", name=tname)
            for j in row:
                g.add_edge(node, j, weight=1.0)
        g.targetNames.append(tname)
        g.targetNodes[tname] = list(trows)
    return g


def csr(rows, index):
    ptr, nbr = [0], []
    for row in rows.values():
        nbr.extend(index[x] for x in row)
        ptr.append(len(nbr))
    return np.array(ptr, dtype=np.int32), np.array(nbr, dtype=np.int32)


def call(fn, *a, **k):
    """('ok', result) or ('raises', exception class name)"""
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return "ok", fn(*a, **k)
    except Exception as e:  # noqa: BLE001 -- the exception type is the recorded result
        return "raises", type(e).__name__


def fixture_cases(gr, out):
    specs = [("small", "mapping_small.npz", ["ME", "IG"]), ("c1", "c1_3k.npz", ["ME"])]
    rng = np.random.default_rng(7)
    for tag, fn, tnames in specs:
        d = np.load(os.path.join(GOLD, fn))
        ref_nodes = [str(x) for x in d["ref_graph_nodes"]]
        ref_rows = rows_of(ref_nodes, d["ref_graph_src"], d["ref_graph_dst"])
        index = {n: i for i, n in enumerate(ref_nodes)}
        t_rows = {t: rows_of([str(x) for x in d["t_%s_graph_nodes" % t]], d["t_%s_graph_src" % t], d["t_%s_graph_dst" % t])
                  for t in tnames}
        g = load_graph(gr, "WT", ref_rows, t_rows)
        out["%s_ref_nodes" % tag] = np.array(ref_nodes)
        out["%s_ref_ptr" % tag], out["%s_ref_nbr" % tag] = csr(ref_rows, index)
        for t in tnames:
            p = "%s_%s" % (tag, t)
            out[p + "_t_nodes"] = np.array(list(t_rows[t]))
            out[p + "_t_ptr"], out[p + "_t_nbr"] = csr(t_rows[t], index)
            fill = g.get_mapping_specificity(t, fill_na=True)
            nofill = g.get_mapping_specificity(t, fill_na=False)
            assert list(fill) == list(t_rows[t]) == list(nofill)
            out[p + "_spec_fill"] = np.array(list(fill.values()), dtype=np.float64)
            out[p + "_spec_nofill"] = np.array(list(nofill.values()), dtype=np.float64)
            for incl in (False, True):
                rs = g.get_ref_specificity(t, fill, incl_unmapped=incl)
                q = p + "_refspec%s" % ("_incl" if incl else "")
                out[q + "_nodes"] = np.array(list(rs))
                out[q + "_vals"] = np.array([float(v) for v in rs.values()], dtype=np.float64)
            # contiguous path lengths: the tutorial's score-sorted lists, random lists, a repeated node
            sc = g.get_mapping_score(t, sorted_names_only=True)
            lists = [sc[:25], sc[:200], sc[::-1][:50], list(rng.choice(ref_nodes, 40)), [ref_nodes[3], ref_nodes[3], ref_nodes[9]],
                     [ref_nodes[5]], []]
            vals = []
            for nodes in lists:
                kind, v = call(g.calc_contiguous_spl, nodes)
                assert kind == "ok", v
                vals.append(v)
            out[p + "_cspl_lists"] = np.array(json.dumps([[index[x] for x in nodes] for nodes in lists]))
            out[p + "_cspl_vals"] = np.array(vals, dtype=np.float64)
            print("  %s: %d target nodes, %d NaN before fill" % (p, len(fill), int(np.isnan(out[p + "_spec_nofill"]).sum())))


def quirk_cases(gr):
    """hand-built graphs; node lists are in load order"""
    R = ["r%d_R" % i for i in range(8)]
    cases = []
    # path r0-r1-r2-r3-r4 with a self-loop on r1, a duplicate arc r0->r1, one-way rows (r2 lists r3, r3 lists nobody),
    # a branch r2-r5-r6 and an isolated r7
    ref_rows = {R[0]: [R[1], R[1]], R[1]: [R[1], R[0], R[2]], R[2]: [R[3], R[5]], R[3]: [], R[4]: [R[3]], R[5]: [R[6]],
                R[6]: [R[5]], R[7]: []}
    targets = {
        "T": {"t0_T": [R[0]], "t1_T": [R[0], R[4]], "t2_T": [R[1], R[2], R[1], R[6]], "t3_T": [], "t4_T": [R[1], R[1]]},
        "U": {"u0_U": [R[0], R[2]], "u1_U": [R[3]], "u2_U": [R[6], R[4], R[0]]},
        "V": {"v0_V": [R[0], R[1]], "v1_V": [R[0], R[7]]},
        "W": {},
    }
    g = load_graph(gr, "R", ref_rows, targets)
    calls = []
    for t in targets:
        for fill in (True, False):
            calls.append({"method": "mapping_specificity", "target": t, "fill_na": fill,
                          "result": call(g.get_mapping_specificity, t, fill_na=fill)})
    kind, spec_t = call(g.get_mapping_specificity, "T", fill_na=False)
    for incl in (False, True):
        calls.append({"method": "ref_specificity", "target": "T", "values": spec_t, "incl_unmapped": incl,
                      "result": call(g.get_ref_specificity, "T", spec_t, incl_unmapped=incl)})
    calls.append({"method": "ref_specificity", "target": "U", "values": {"u0_U": 1.5, "u1_U": 0.1, "u2_U": 0.2},
                  "incl_unmapped": False,
                  "result": call(g.get_ref_specificity, "U", {"u0_U": 1.5, "u1_U": 0.1, "u2_U": 0.2})})
    for nodes in ([R[0], R[4], R[6], R[0]], [R[0]], [], [R[1], R[1], R[2]], [R[0], R[7]]):
        calls.append({"method": "contiguous_spl", "nodes": nodes, "result": call(g.calc_contiguous_spl, nodes)})
    calls.append({"method": "mapping_specificity", "target": "missing", "fill_na": True,
                  "result": call(g.get_mapping_specificity, "missing")})
    cases.append({"ref_rows": list(ref_rows.items()), "targets": {t: list(r.items()) for t, r in targets.items()},
                  "calls": calls})
    return cases


def main():
    gr = load_graph_module()
    out = {}
    fixture_cases(gr, out)
    out["quirks"] = np.array(json.dumps(quirk_cases(gr)))
    fn = os.path.join(GOLD, "paths.npz")
    np.savez_compressed(fn, **out)
    print("wrote %s (%d bytes)" % (fn, os.path.getsize(fn)))


if __name__ == "__main__":
    sys.exit(main())
