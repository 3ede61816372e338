#!/usr/bin/env python3
"""Writes tests/golden/potential.npz: the graphs the potential tests run on, their right-hand sides, and what the dense
route gives on them -- the reference's own Graph.calc_diff_potential (nabo/_graph.py:918-954), numpy.linalg.pinv of
I - A/D from the tests' yardstick (tests/_potential_ref.py), the smallest non-zero eigenvalue of K, and the measured
distances between the yardstick's best attainable iterate and both.

TEST INFRASTRUCTURE ONLY, run where a checkout of the reference is at hand, with an interpreter that has networkx and
pandas (networkx 2.6.3, pandas 2.3.3, numpy 1.26.4 when the file was written):

    NABO_REFERENCE=/path/to/nabo-checkout python tools/gen_golden_potential.py

The reference's nabo/_graph.py is loaded BY FILE PATH (as tools/gen_golden_paths.py does) and its Graph is filled node by
node and row by row in the order Graph.load_from_h5 would (nabo/_graph.py:93-107).  Only DATA is written.  Per graph G
and right-hand side R in ("ones", "r"):

    G_ptr, G_nbr           the graph as listed (int32), self-loops and all
    G_r                    the right-hand side "r" ("ones" is r = None)
    G_R_pinv               pinv(I - A/D) r from the yardstick's dense matrix
    G_R_ref                the reference's values, by node id
    G_R_delta_pinv, _ref   || yardstick(best attainable) - pinv ||_2, || yardstick(best attainable) - reference ||_2
    G_R_iterations         the yardstick's iterations to tol = 1e-10
    G_lambda2              the smallest non-zero eigenvalue of K
"""
import importlib.util
import os
import re
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
REF = os.environ.get("NABO_REFERENCE")
GOLD = os.path.join(REPO, "tests", "golden")
sys.path.insert(0, os.path.join(REPO, "tests"))
import _community_ref as cr  # noqa: E402
import _potential_ref as pr  # noqa: E402


def load_graph_module():
    if not REF:
        sys.exit("set NABO_REFERENCE to a checkout of the reference (the directory that holds nabo/_graph.py)")
    spec = importlib.util.spec_from_file_location("nabo_ref_graph", os.path.join(REF, "nabo", "_graph.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def reference_values(gr, names, ptr, nbr, r):
    """Graph.calc_diff_potential on the graph as listed: values by node id"""
    g = gr.Graph()
    for i, node in enumerate(names):
        g.add_node(node, kind="reference", name="R")
        for j in nbr[ptr[i]:ptr[i + 1]].tolist():
            g.add_edge(node, names[j], weight=1.0)
    g.refName = "R"
    g.refNodes = list(names)
    g.refG = g.subgraph(g.refNodes)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = g.calc_diff_potential(None if r is None else {x: float(v) for x, v in zip(names, r)})
    assert sorted(res) == sorted(names)
    return np.array([res[x] for x in names], dtype=np.float64)


def long_threshold():
    src = open(os.path.join(REPO, "nabo_amd", "csrc", "potential.hip")).read()
    return int(re.search(r"PT_LONG = (\d+);", src).group(1)), int(re.search(r"PT_ROWS = (\d+);", src).group(1))


def graphs(thr, rows):
    g = {}
    for n in (96, 400):
        ptr, nbr, _ = cr.blob_snn_graph(n=n, centres=4)
        g["blob%d" % n] = (ptr, nbr)
    d = np.load(os.path.join(GOLD, "community.npz"))          # the 3 000-node blob graph of the community tests
    g["blob3000"] = (d["ptr"].astype(np.int64), d["nbr"].astype(np.int64))
    g["hub"] = pr.hub_graph(thr)
    for n in sorted({257, rows - 1, rows + 1}):
        g["path%d" % n] = pr.path_graph(n)
    g.update(pr.small_graphs())
    # the reference graph of tests/golden/mapping_small.npz, rows in the file's order
    d = np.load(os.path.join(GOLD, "mapping_small.npz"))
    nodes = [str(x) for x in d["ref_graph_nodes"]]
    pos = {x: i for i, x in enumerate(nodes)}
    g["mapping_small"] = pr.csr_of_edges(len(nodes), [(pos[str(a)], pos[str(b)]) for a, b in zip(d["ref_graph_src"], d["ref_graph_dst"])])
    return g, nodes


def main():
    gr = load_graph_module()
    thr, rows = long_threshold()
    out = {"long_threshold": np.int64(thr), "block_rows": np.int64(rows)}
    gs, map_nodes = graphs(thr, rows)
    out["names"] = np.array(list(gs))
    out["mapping_small_nodes"] = np.array(map_nodes)
    for at, (name, (ptr, nbr)) in enumerate(gs.items()):
        G = pr.Graph(ptr, nbr)
        n = G.n
        names = map_nodes if name == "mapping_small" else ["n%d_R" % i for i in range(n)]
        r = np.random.default_rng(100 + at).normal(size=n) * 3.0 - 0.5          # both signs
        out[name + "_ptr"], out[name + "_nbr"], out[name + "_r"] = ptr.astype(np.int32), nbr.astype(np.int32), r
        out[name + "_lambda2"] = np.float64(pr.lambda2(G))
        P = np.linalg.pinv(G.dense_L())
        for tag, rv in (("ones", None), ("r", r)):
            pinv = np.dot(P, np.ones(n) if rv is None else rv)
            ref = reference_values(gr, names, ptr, nbr, rv)
            b = pr.rhs(G, rv)
            best = pr.centre(G, pr.best_attainable(G, b)[0])
            run = pr.PCG(G, b, 1e-10, 10000).run()
            key = "%s_%s_" % (name, tag)
            out[key + "pinv"], out[key + "ref"] = pinv, ref
            out[key + "delta_pinv"] = np.float64(np.linalg.norm(best - pinv))
            out[key + "delta_ref"] = np.float64(np.linalg.norm(best - ref))
            out[key + "iterations"] = np.int64(run.it)
            assert run.status == pr.CONVERGED, (name, tag, run.status)
            print("%-20s %-4s n=%5d comps=%3d loops=%4d lambda2=%.3g: %4d iterations; best - pinv %.3g, best - reference %.3g, "
                  "pinv - reference %.3g (max |V| %.3g)" % (name, tag, n, len(G.roots), int(G.loop.sum()), out[name + "_lambda2"], run.it,
                                                           out[key + "delta_pinv"], out[key + "delta_ref"], np.linalg.norm(pinv - ref),
                                                           np.abs(pinv).max()))
    fn = os.path.join(GOLD, "potential.npz")
    np.savez_compressed(fn, **out)
    print("wrote %s (%d bytes)" % (fn, os.path.getsize(fn)))


if __name__ == "__main__":
    sys.exit(main())
