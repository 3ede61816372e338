"""Hop distances on the reference graph on the MI355X (nabo_refgraph_*, nabo_amd._paths): bit parity with the
reference's Graph methods (tests/golden/paths.npz), both tiers forced on awkward graphs against the tests' own BFS,
and a 200k-cell SNN graph built by the product."""
import json
import os
import subprocess

import numpy as np
import pytest

import _paths_oracle as orc
from test_mapping import _interpreter

HERE = os.path.dirname(os.path.abspath(__file__))
OPTIONS = [None, {"local_capacity": 0}, {"local_capacity": 6}]


def _dg(ptr, nbr, options=None):
    from nabo_amd._paths import _DeviceGraph
    return _DeviceGraph(ptr, nbr, 0, options)


def _same(a, b):
    return list(a) == list(b) and np.array_equal(np.array(list(a.values()), dtype=np.float64),
                                                 np.array(list(b.values()), dtype=np.float64), equal_nan=True)


@pytest.mark.gpu
@pytest.mark.parametrize("options", OPTIONS)
def test_fixture_parity(gpu_lib, golden, options):
    from nabo_amd._paths import _contiguous, _specificity
    d = golden("paths")
    for tag, t in (("small", "ME"), ("small", "IG"), ("c1", "ME")):
        ref = [str(x) for x in d[tag + "_ref_nodes"]]
        g = _dg(d[tag + "_ref_ptr"], d[tag + "_ref_nbr"], options)
        try:
            p = "%s_%s" % (tag, t)
            nodes = [str(x) for x in d[p + "_t_nodes"]]
            for fill, key in ((True, "_spec_fill"), (False, "_spec_nofill")):
                got = _specificity(g, ref, nodes, d[p + "_t_ptr"], d[p + "_t_nbr"], fill)
                assert _same(got, dict(zip(nodes, d[p + key].tolist()))), (p, fill)
            for lst, v in zip(json.loads(str(d[p + "_cspl_lists"])), d[p + "_cspl_vals"].tolist()):
                got = _contiguous(g, ref, lst)
                assert got == v or (got != got and v != v), (p, lst)
        finally:
            g.close()


@pytest.mark.gpu
def test_quirks_match_reference(gpu_lib, golden):
    from nabo_amd._paths import _contiguous, _ref_specificity_rows, _specificity
    case = json.loads(str(golden("paths")["quirks"]))[0]
    ref = [r for r, _ in case["ref_rows"]]
    pos = {n: i for i, n in enumerate(ref)}
    ptr = np.concatenate([[0], np.cumsum([len(row) for _, row in case["ref_rows"]])])
    nbr = np.array([pos[x] for _, row in case["ref_rows"] for x in row], dtype=np.int64)
    targets = {}
    for t, rows in case["targets"].items():
        tp = np.concatenate([[0], np.cumsum([len(r) for _, r in rows])]).astype(np.int64)
        tn = np.array([pos[x] for _, r in rows for x in r], dtype=np.int64)
        targets[t] = ([n for n, _ in rows], tp, tn)
    for options in OPTIONS:
        g = _dg(ptr, nbr, options)
        try:
            for c in case["calls"]:
                kind, want = c["result"]
                try:
                    if c["method"] == "mapping_specificity":
                        if c["target"] not in targets:
                            raise KeyError(c["target"])
                        got = _specificity(g, ref, *targets[c["target"]], c["fill_na"])
                    elif c["method"] == "ref_specificity":
                        nodes, tp, tn = targets[c["target"]]
                        got = _ref_specificity_rows(ref, pos, len(ref), nodes, tp, tn, c["values"], c["incl_unmapped"])
                    else:
                        got = _contiguous(g, ref, [pos[n] for n in c["nodes"]])
                except (KeyError, ValueError) as e:
                    # the reference raises networkx.NetworkXNoPath where this build raises ValueError
                    assert kind == "raises", (c, e)
                    assert type(e).__name__ == want or (want == "NetworkXNoPath" and "no path" in str(e)), (c, e)
                    continue
                assert kind == "ok", c
                if isinstance(want, dict):
                    assert _same(got, want), (c, got)
                else:
                    assert got == want or (got != got and want != want), (c, got)
        finally:
            g.close()


# ---- both tiers on awkward graphs ---------------------------------------------------------------------------------
def _csr(n, arcs):
    arcs = sorted(arcs, key=lambda a: a[0])
    ptr = np.zeros(n + 1, dtype=np.int64)
    for a, _ in arcs:
        ptr[a + 1] += 1
    return np.cumsum(ptr), np.array([b for _, b in arcs], dtype=np.int64)


def _graphs():
    rng = np.random.default_rng(5)
    out = {}
    for n in (301, 300):
        out["path%d" % n] = (n, [(i, i + 1) for i in range(n - 1)])
        out["cycle%d" % n] = (n, [(i, (i + 1) % n) for i in range(n)])
    # star: hub 0 of degree 10 000, a tail 1-10001-10002-... on one leaf
    out["star"] = (10011, [(0, i) for i in range(1, 10001)] + [(1, 10001)] + [(10000 + i, 10001 + i) for i in range(1, 10)])
    # two components and isolated nodes
    out["split"] = (120, [(i, i + 1) for i in range(49)] + [(60 + i, 61 + i) for i in range(40)])
    # one-way rows, duplicate arcs, self-loops on a sparse random graph
    n = 2000
    a = rng.integers(0, n, 5000)
    b = rng.integers(0, n, 5000)
    arcs = list(zip(a.tolist(), b.tolist())) + [(int(x), int(y)) for x, y in zip(a[:800], b[:800])] + [(i, i) for i in range(0, n, 7)]
    out["messy"] = (n, arcs)
    return out


def _groups(n, rng):
    sizes = [0, 1, 2, 2, 3, 5, 8, 11, 64, 65, 300, 0, 2]
    grp = [rng.integers(0, n, s).tolist() for s in sizes]
    grp.append([0, n - 1])                                   # the far ends
    grp.append([n // 2, n // 2, 3, n // 2, 3])               # repeated members
    grp.append([5] * 64)                                     # one node 64 times
    return grp


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(_graphs()))
def test_forced_tiers_against_bfs(gpu_lib, name):
    n, arcs = _graphs()[name]
    ptr, nbr = _csr(n, arcs)
    uptr, ucol = orc.undirected(n, ptr, nbr)
    rng = np.random.default_rng(11)
    grp = _groups(n, rng)
    gp = np.concatenate([[0], np.cumsum([len(x) for x in grp])]).astype(np.int64)
    mem = np.array([v for x in grp for v in x], dtype=np.int64)
    ws, wu, wp = orc.group_hops(uptr, ucol, gp, mem)
    with_pairs = sum(1 for x in grp if len(x) >= 2)
    small = sum(1 for x in grp if 2 <= len(x) <= 64)
    for options in OPTIONS:
        g = _dg(ptr, nbr, options)
        try:
            s, u, ph = g.group_hops(gp, mem, pair_hops=True)
            st = g.last_stats()
            s2, u2 = g.group_hops(gp, mem)
        finally:
            g.close()
        assert np.array_equal(ph, wp), (name, options)
        assert np.array_equal(s, ws) and np.array_equal(u, wu), (name, options)
        assert np.array_equal(s2, ws) and np.array_equal(u2, wu), (name, options)
        assert st["local_groups"] + st["global_groups"] == with_pairs, st
        if options is None:
            assert st["local_groups"] > 0, st                # the local tier answered
        elif options["local_capacity"] == 0:
            assert st["local_groups"] == 0 and st["global_groups"] == with_pairs and st["sweeps"] > 0, st
        else:
            # a 6-node table overflows partway through every search that needs more
            assert st["global_groups"] > with_pairs - small and st["sweeps"] > 0, st
    if name.startswith("path"):
        assert wp.max() >= 250                               # distances into the hundreds


# ---- a product-built SNN graph --------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_scale_200k_snn_graph(gpu_lib):
    import nabo_amd
    from nabo_amd._mapping import snn_edges
    from nabo_amd._synth import pca_like
    n, k = 200000, 11
    ref = pca_like(n, 30, seed=41)
    r_idx, _ = nabo_amd.knn(ref, ref, k, metric=nabo_amd.EUCLIDEAN, drop_first=True)
    et, ej, _ = snn_edges(r_idx, r_idx, k)
    ptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(et, minlength=n), out=ptr[1:])
    nbr = ej[np.argsort(et, kind="stable")]
    tgt = pca_like(n, 30, seed=43)
    t_idx, _ = nabo_amd.knn(tgt, ref, k, metric=nabo_amd.EUCLIDEAN)
    tt, tj, _ = snn_edges(t_idx, r_idx, k)
    # groups: a target cell's mapped reference cells (each once, in row order)
    gp = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(tt, minlength=n), out=gp[1:])
    mem = tj[np.argsort(tt, kind="stable")]
    res = {}
    for options in OPTIONS:
        g = _dg(ptr, nbr, options)
        try:
            s, u = g.group_hops(gp, mem)
            st = g.last_stats()
            nodes = g.last_local_nodes(n) if options is None else None
        finally:
            g.close()
        res[json.dumps(options)] = (s, u, st, nodes)
    s0, u0, st0, nodes = res["null"]
    for key, (s, u, st, _) in res.items():
        assert np.array_equal(s, s0) and np.array_equal(u, u0), key
    # both tiers ran; between them they answered every group with a pair
    assert st0["local_groups"] > 0 and st0["global_groups"] > 0, st0
    assert st0["local_groups"] + st0["global_groups"] == int((np.diff(gp) >= 2).sum()), st0
    # 2 000 sampled groups, the largest-ball ones (handed on, or the largest local tables) included
    rng = np.random.default_rng(3)
    big = np.argsort(np.where(nodes < 0, np.iinfo(np.int32).max, nodes))[-60:]
    pick = np.unique(np.concatenate([big, rng.choice(n, 1940, replace=False)]))
    uptr, ucol = orc.undirected(n, ptr, nbr)
    for gi in pick.tolist():
        d = orc.pair_hops(uptr, ucol, mem[gp[gi]:gp[gi + 1]])
        assert s0[gi] == sum(x for x in d if x >= 0) and u0[gi] == sum(1 for x in d if x < 0), gi


@pytest.mark.gpu
def test_file_level_functions_both_layouts(gpu_lib):
    py = _interpreter()
    if py is None:
        pytest.skip("no interpreter with h5py in this image")
    r = subprocess.run([py, os.path.join(HERE, "_paths_case.py")], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       universal_newlines=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][len("RESULT "):])
    assert res["checked"] >= 40 and res["differ"] == [], res
