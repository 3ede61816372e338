"""Plain-Python restatement of the classification and ring steps (no GPU), and the checks of every golden case
(tests/golden/classify.npz, tools/gen_golden_classify.py) with the device steps passed in: the CPU tests pass this
restatement, the GPU tests the library."""
import json
from collections import Counter

import numpy as np

import _paths_oracle as orc


def classify(ref_cluster, n_clusters, ptr, nbr, w, weight_frac, min_degree, min_weight, details=False):
    """(label, counts) as nabo_classify_targets returns them; details=True: (label, best, total, counts, tied) with
    tied[t] = two or more clusters share the best weight AND it passes the threshold"""
    n_t = len(ptr) - 1
    label = np.full(n_t, -1, dtype=np.int32)
    best, total = np.zeros(n_t), np.zeros(n_t)
    tied = np.zeros(n_t, dtype=bool)
    ref_cluster = np.asarray(ref_cluster).tolist()
    nbr_l, w_l = np.asarray(nbr).tolist(), np.asarray(w, dtype=np.float64).tolist()
    for t in range(n_t):
        merged = {}
        for e in range(int(ptr[t]), int(ptr[t + 1])):
            merged[nbr_l[e]] = w_l[e]                      # first position, last weight: what nx.Graph.add_edge does
        sums = [0] * n_clusters
        tot = 0
        for r, x in merged.items():
            if x > min_weight and ref_cluster[r] >= 0:
                sums[ref_cluster[r]] += x
            tot += x
        top = max(sums)
        c = sums.index(top)                                # the lowest cluster id among the best
        best[t], total[t] = top, tot
        if len(merged) >= min_degree and top > weight_frac * tot:
            label[t] = c
            tied[t] = sums.count(top) > 1
    counts = np.bincount(np.where(label < 0, n_clusters, label), minlength=n_clusters + 1).astype(np.int64)
    return (label, best, total, counts, tied) if details else (label, counts)


def set_levels(uptr, ucol, sets, max_level=-1):
    """int32 [n_sets, n]: hops to the nearest member of each set on the undirected graph (uptr, ucol)"""
    n = uptr.shape[0] - 1
    out = np.full((len(sets), n), -1, dtype=np.int32)
    for s, mem in enumerate(sets):
        front = np.unique(np.asarray(mem, dtype=np.int64))
        out[s, front] = 0
        level = 0
        while front.size and (max_level < 0 or level < max_level):
            level += 1
            deg = uptr[front + 1] - uptr[front]
            idx = np.repeat(uptr[front] - np.concatenate([[0], np.cumsum(deg)[:-1]]), deg) + np.arange(int(deg.sum()))
            nb = np.unique(ucol[idx])
            nb = nb[out[s, nb] < 0]
            out[s, nb] = level
            front = nb
    return out


def levels_step(n, ptr, nbr):
    """the ring functions' device step on the restatement: (seed positions, k_dist) -> level [n]"""
    uptr, ucol = orc.undirected(n, ptr, nbr)
    return lambda seeds, k: set_levels(uptr, ucol, [seeds], k)[0]


# ---- the golden cases, device steps passed in -----------------------------------------------------------------------
def _same_labels(got, want, tied_idx, own):
    """labels equal to the reference's except at deciding ties, where this build's rule (`own`) holds"""
    got, want = list(got), list(want)
    tied_idx = set(int(i) for i in tied_idx)
    return all((g == own[i]) if i in tied_idx else (g == w) for i, (g, w) in enumerate(zip(got, want)))


def check_fixtures(paths, gold, classify_step, make_levels_step):
    """every fixture case of classify.npz; returns the number of cases checked"""
    from nabo_amd._classify import (_classify_rows, _de_groups, _k_path_from_rings, _mapped_cells, _rings_from_levels,
                                    _valid_nodes)
    from nabo_amd._score import mapping_score_from_edges
    checked = 0
    graphs = {}
    for tag in ("small", "c1"):
        ref = [str(x) for x in paths[tag + "_ref_nodes"]]
        ptr, nbr = paths[tag + "_ref_ptr"].astype(np.int64), paths[tag + "_ref_nbr"].astype(np.int64)
        src = np.repeat(np.arange(len(ref)), np.diff(ptr))
        selfloop = np.zeros(len(ref), dtype=bool)
        selfloop[src[src == nbr]] = True
        lab, unnamed = gold[tag + "_clusters"], gold[tag + "_unnamed"]
        variants = {"full": {n: int(lab[i]) for i, n in enumerate(ref)},
                    "partial": {n: int(lab[i]) for i, n in enumerate(ref) if not unnamed[i]}}
        graphs[tag] = (ref, {n: i for i, n in enumerate(ref)}, selfloop, variants, make_levels_step(len(ref), ptr, nbr))

    def target(tag, t):
        p = "%s_%s" % (tag, t)
        return ([str(x) for x in paths[p + "_t_nodes"]], paths[p + "_t_ptr"].astype(np.int64),
                paths[p + "_t_nbr"].astype(np.int64), gold[p + "_t_w"])

    from nabo_amd._classify import _imported_clusters
    for c in json.loads(str(gold["cases"])):
        ref, pos, _, variants, _ = graphs[c["tag"]]
        t_nodes, tp, tn, tw = target(c["tag"], c["target"])
        named = variants[c["variant"]]
        cd = _imported_clusters(ref, named) if c["form"] == "clusters" else named
        na = "NA" if c["form"] == "clusters" else "unk"
        args = (ref, pos, len(ref), t_nodes, tp, tn, tw, c["weight_frac"], c["min_degree"], c["min_weight"], cd, na)
        got = _classify_rows(*args, False, classify_step)
        own = _classify_rows(*args, False, classify)            # this build's rule at the ties
        tied = gold[c["key"] + "_tied"]
        assert list(got) == t_nodes, c["key"]
        assert _same_labels([str(v) for v in got.values()], [str(x) for x in gold[c["key"] + "_labels"]], tied,
                            [str(v) for v in own.values()]), c["key"]
        cnt = _classify_rows(*args, True, classify_step)
        mine = {str(k): int(v) for k, v in cnt.items()}
        if tied.size == 0:
            assert mine == c["counts"], (c["key"], mine, c["counts"])
        else:
            tally = Counter(str(v) for v in got.values())
            assert set(mine) == set(c["counts"]) and all(mine[k] == tally.get(k, 0) for k in mine), c["key"]
        checked += 1
    for c in json.loads(str(gold["rings"])):
        ref, pos, selfloop, _, levels = graphs[c["tag"]]
        nodes = [ref[i] for i in c["nodes"]]
        level = levels(c["nodes"], c["k_dist"]) if c["k_dist"] > 0 else np.full(len(ref), -1, dtype=np.int32)
        rings = _rings_from_levels(level, selfloop, ref, pos, nodes, c["k_dist"])
        got = [pos[x] for x in _k_path_from_rings(rings, c["full_trail"], c["trail_start"])]
        assert (got if c["as_given"] else sorted(got)) == c["result"], c
        checked += 1
    for c in json.loads(str(gold["de_groups"])):
        ref, pos, selfloop, variants, levels = graphs[c["tag"]]
        t_nodes, tp, tn, tw = target(c["tag"], c["target"])
        kw = dict(c["kwargs"])
        sc = mapping_score_from_edges(len(ref), tn, tw, len(t_nodes), 0, -np.inf)
        valid = {n: v for n, v in zip(ref, sc.tolist()) if v >= kw["min_score"]}

        def k_path(nodes, k, full, start):
            seeds = [pos[x] for x in nodes]
            level = levels(seeds, k) if k > 0 else np.full(len(ref), -1, dtype=np.int32)
            return _k_path_from_rings(_rings_from_levels(level, selfloop, ref, pos, nodes, k), full, start)

        import contextlib
        import io
        with contextlib.redirect_stdout(io.StringIO()):
            nodes_ok = _valid_nodes(ref, kw.get("from_clusters"), _imported_clusters(ref, variants["full"]))
            got = _de_groups(ref, nodes_ok, valid, k_path, kw["node_dist"], kw.get("full_trail", False),
                             kw.get("trail_start", 1), kw.get("stringent_control", False))
        want = c["result"]
        if want is None:
            assert got is None, c["kwargs"]
        else:
            code = {"Other": 0, "Test": 1, "Control": 2}
            assert list(got["de_group"]) == ref and [code[v] for v in got["de_group"].values()] == want["de_group"], c["kwargs"]
            assert got["deTestCells"] == want["deTestCells"] and sorted(got["deCtrlCells"]) == want["deCtrlCells"], c["kwargs"]
        checked += 1
    for c in json.loads(str(gold["mapped_cells"])):
        ref, pos, _, _, _ = graphs[c["tag"]]
        t_nodes, tp, tn, _ = target(c["tag"], c["target"])
        assert _mapped_cells(pos, "WT", t_nodes, tp, tn, c["ref_cells"], c["remove_suffix"]) == c["result"], c
        checked += 1
    return checked


def quirk_graph(gold):
    """(case, ref names, pos, ref ptr, ref nbr, {target: (nodes, ptr, nbr, w)})"""
    case = json.loads(str(gold["quirks"]))
    ref = [r for r, _ in case["ref_rows"]]
    pos = {n: i for i, n in enumerate(ref)}
    ptr = np.concatenate([[0], np.cumsum([len(row) for _, row in case["ref_rows"]])]).astype(np.int64)
    nbr = np.array([pos[x] for _, row in case["ref_rows"] for x, _ in row], dtype=np.int64)
    targets = {}
    for t, rows in case["targets"].items():
        tp = np.concatenate([[0], np.cumsum([len(r) for _, r in rows])]).astype(np.int64)
        tn = np.array([pos[x] for _, r in rows for x, _ in r], dtype=np.int64)
        tw = np.array([x for _, r in rows for _, x in r], dtype=np.float64)
        targets[t] = ([n for n, _ in rows], tp, tn, tw)
    return case, ref, pos, ptr, nbr, targets


def check_quirks(gold, classify_step, make_levels_step):
    """every recorded call on the hand-built graph: result or exception class; returns the number checked"""
    from nabo_amd._classify import (_classify_rows, _cluster_ids, _imported_clusters, _k_path_from_rings, _mapped_cells,
                                    _rings_from_levels, _valid_nodes, _validate_clusters)
    case, ref, pos, ptr, nbr, targets = quirk_graph(gold)
    src = np.repeat(np.arange(len(ref)), np.diff(ptr))
    selfloop = np.zeros(len(ref), dtype=bool)
    selfloop[src[src == nbr]] = True
    levels = make_levels_step(len(ref), ptr, nbr)
    checked = 0
    for c in case["calls"]:
        kind, want = c["result"]
        kw = dict(c["kwargs"])
        try:
            if c["method"] == "classify_target":
                cd = kw.get("cluster_dict")
                if cd is None:
                    cd = _imported_clusters(ref, kw.get("clusters"))
                    _validate_clusters(cd)
                t_nodes, tp, tn, tw = targets[kw["target"]]
                args = (ref, pos, len(ref), t_nodes, tp, tn, tw, kw.get("weight_frac", 0.5), kw.get("min_degree", 2),
                        kw.get("min_weight", 0.1), cd, kw.get("na_label", "NA"), kw.get("ret_counts", False))
                got = {str(k): v for k, v in _classify_rows(*args, classify_step).items()}
                # deciding ties follow this build's rule (lowest cluster id), everything else the reference
                labels, rc = _cluster_ids(ref, pos, len(ref), cd)
                tied = classify(rc, len(labels), tp, tn, tw, args[7], args[8], args[9], details=True)[4] if labels else []
                if not kw.get("ret_counts", False):
                    own = _classify_rows(*args, classify)
                    for i in np.nonzero(tied)[0].tolist():
                        assert got[t_nodes[i]] == own[t_nodes[i]], (c, t_nodes[i])
                        want = dict(want, **{t_nodes[i]: got[t_nodes[i]]})
                elif np.any(tied):
                    # counts under a deciding tie: the reference's keys, and the tally of this build's own labels
                    by_node = _classify_rows(*(args[:-1] + (False,)), classify_step)
                    tally = Counter(str(v) for v in by_node.values())
                    assert set(got) == set(want) and all(got[k] == tally.get(k, 0) for k in got), (c, got)
                    want = got
            elif c["method"] == "k_path_neighbours":
                nodes, k = kw["nodes"], kw["k_dist"]
                seeds = [pos[x] for x in nodes if x in pos]
                level = levels(seeds, k) if k > 0 else np.full(len(ref), -1, dtype=np.int32)
                got = _k_path_from_rings(_rings_from_levels(level, selfloop, ref, pos, nodes, k), kw["full_trail"], kw["trail_start"])
                if not (k == 0 and not kw["full_trail"]):
                    got = sorted(got)
            elif c["method"] == "mapped_cells":
                if kw["target"] not in targets:
                    raise ValueError("ERROR: %s not present in graph!" % kw["target"])
                t_nodes, tp, tn, _ = targets[kw["target"]]
                got = _mapped_cells(pos, "R", t_nodes, tp, tn, kw["ref_cells"], kw.get("remove_suffix", True))
            else:
                got = _valid_nodes(ref, kw["from_clusters"], _imported_clusters(ref, case["imported"]))
        except (KeyError, ValueError, TypeError) as e:
            assert kind == "raises" and type(e).__name__ == want, (c, repr(e))
            checked += 1
            continue
        assert kind == "ok" and got == want, (c, got)
        checked += 1
    return checked
