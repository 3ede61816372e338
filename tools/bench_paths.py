"""Mapping specificity over every target node of a large mapping: the two tiers of nabo_refgraph_group_hops, split.
Same setup as tools/bench_mapping.py (pca_like reference and target, dense input, columnar layouts); needs h5py (run
with /opt/conda/bin/python3.9 in this image).

    python tools/bench_paths.py [n_ref n_target d k] [--nx N]

Prints one JSON line: Mapping time, RefGraph upload, specificity wall time and per tier (from last_stats), how many
groups each tier answered, a histogram of the local tier's table sizes (nodes visited per group), the CSR bytes the
local tier gathered and their rate, and networkx's get_mapping_specificity loop on N sampled targets (default 500)
extrapolated to all of them -- skipped when networkx is absent."""
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nabo_amd  # noqa: E402
from nabo_amd import _paths  # noqa: E402
from nabo_amd._synth import pca_like  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
n_nx = int(sys.argv[sys.argv.index("--nx") + 1]) if "--nx" in sys.argv else 500
if "--nx" in sys.argv:
    args.remove(str(n_nx))
n_ref, n_tgt, d, k = (int(a) for a in (args + ["1000000", "1000000", "50", "15"][len(args):]))
tmp = tempfile.mkdtemp(prefix="nabo_bp_")
out = {"n_ref": n_ref, "n_target": n_tgt, "d": d, "k": k}
try:
    nabo_amd.write_dense_pca(os.path.join(tmp, "ref.h5"), "data", ["R%07d" % i for i in range(n_ref)], pca_like(n_ref, d + 5, seed=1001))
    nabo_amd.write_dense_pca(os.path.join(tmp, "tgt.h5"), "data", ["T%07d" % i for i in range(n_tgt)], pca_like(n_tgt, d + 5, seed=2001))
    fn = os.path.join(tmp, "map.h5")
    t0 = time.perf_counter()
    m = nabo_amd.Mapping(fn, "WT", os.path.join(tmp, "ref.h5"), "data", overwrite=True, layout="columnar", graph_layout="columnar")
    m.set_parameters(d, k, 0.25, 500)
    m.make_ref_graph()
    m.map_target("ME", os.path.join(tmp, "tgt.h5"), "data")
    out["s_mapping"] = round(time.perf_counter() - t0, 2)

    t0 = time.perf_counter()
    g = nabo_amd.RefGraph(fn, "WT")
    out["s_refgraph_open"] = round(time.perf_counter() - t0, 2)
    import h5py
    with h5py.File(fn, "r") as h5:
        t_nodes, tptr, tnbr = _paths._target_rows(h5, "ME", g.pos)
    gp, mem = _paths._mapped_sets(tptr, tnbr)
    g._g.group_hops(gp[:1001], mem[:gp[1000]])                 # warm-up (code objects, global-tier buffers)
    t0 = time.perf_counter()
    s, u = g._g.group_hops(gp, mem)
    out["s_group_hops"] = round(time.perf_counter() - t0, 3)
    st = g._g.last_stats()
    out["ms_build_local_global_total"] = [round(x, 1) for x in st["ms"]]
    out["groups"] = {"local": st["local_groups"], "global": st["global_groups"],
                     "no_pairs": int((np.diff(gp) < 2).sum()), "sweeps": st["sweeps"], "max_level": st["max_level"]}
    nodes = g._g.last_local_nodes(len(t_nodes))
    loc = nodes[nodes >= 0]
    edges = [0, 8, 16, 32, 64, 128, 256, 512, 1024]
    out["local_nodes_hist"] = {"%d-%d" % (a, b - 1): int(((loc >= a) & (loc < b)).sum()) for a, b in zip(edges[:-1], edges[1:])}
    out["local_nodes_p50_p90_p99_max"] = [int(np.percentile(loc, q)) for q in (50, 90, 99)] + [int(loc.max())] if loc.size else []
    t0 = time.perf_counter()
    spec = g.mapping_specificity("ME", fill_na=True)
    out["s_mapping_specificity_api"] = round(time.perf_counter() - t0, 3)
    assert len(spec) == n_tgt
    # degree of the resident graph: from the CSR the ref group holds (both directions, duplicates merged)
    with h5py.File(fn, "r") as h5:
        from nabo_amd._mapping import read_graph_csr
        uid = h5["name_stash/ref_name"][1].decode()
        _, rptr, rnbr, _ = read_graph_csr(h5[uid + "_graph"], None)
    rows = np.repeat(np.arange(len(rptr) - 1), np.diff(rptr))
    key = np.unique(np.concatenate([rows.astype(np.int64) * n_ref + rnbr, rnbr * n_ref + rows]))
    mean_deg = key.shape[0] / n_ref
    out["ref_arcs_undirected"] = int(key.shape[0])
    out["ref_mean_degree"] = round(mean_deg, 2)
    # CSR bytes the local tier gathered: every table node expanded at most once (two row pointers + its int32 row)
    gathered = float(loc.sum()) * (mean_deg * 4 + 8)
    out["local_csr_bytes_GB"] = round(gathered / 1e9, 3)
    out["local_csr_gather_GBps"] = round(gathered / 1e9 / (st["ms"][1] / 1e3), 1) if st["ms"][1] > 0 else None
    g.close()

    # networkx: the reference's per-pair loop (nabo/_graph.py:811-821) on sampled targets
    try:
        import networkx as nx
    except ImportError:
        nx = None
    if nx is not None and n_nx > 0:
        G = nx.Graph()
        G.add_nodes_from(range(n_ref))
        a, b = key // n_ref, key % n_ref
        G.add_edges_from(zip(a[a <= b].tolist(), b[a <= b].tolist()))
        rng = np.random.default_rng(0)
        pick = rng.choice(len(t_nodes), min(n_nx, len(t_nodes)), replace=False)
        t0 = time.perf_counter()
        for i in pick.tolist():
            tg = mem[gp[i]:gp[i + 1]].tolist()
            spls = [nx.shortest_path_length(G, source=tg[a], target=tg[b]) for a in range(len(tg)) for b in range(len(tg)) if a < b]
            v = float(np.mean(spls)) if spls else float("nan")
            assert v == spec[t_nodes[i]] or (v != v)
        dt = time.perf_counter() - t0
        out["networkx_s_sampled"] = round(dt, 2)
        out["networkx_n_sampled"] = int(len(pick))
        out["networkx_s_extrapolated_all"] = round(dt / len(pick) * len(t_nodes), 0)
    else:
        out["networkx"] = "skipped (not installed)" if nx is None else "skipped (--nx 0)"
finally:
    shutil.rmtree(tmp, ignore_errors=True)
print(json.dumps(out))
