"""Classification and DE groups on the MI355X (nabo_classify_targets, nabo_refgraph_set_levels, nabo_amd._classify):
parity with the reference's Graph methods (tests/golden/classify.npz) for every option set of the resident graph, the
quirk graph, real mapping files in both layouts, a 200k-cell SNN graph built by the product against the tests' plain
restatement, rows at the boundaries of the kernel's stage, set levels on awkward graphs against the tests' BFS, and the
plain-C consumer."""
import json
import os
import subprocess

import numpy as np
import pytest

import _classify_ref as cref
import _paths_oracle as orc
from test_classify_cpu import build_cluster_check
from test_mapping import _interpreter
from test_paths_gpu import OPTIONS, _csr, _graphs

HERE = os.path.dirname(os.path.abspath(__file__))


def _gpu_classify(ref_cluster, n_clusters, ptr, nbr, w, weight_frac, min_degree, min_weight):
    from nabo_amd._classify import _device_classify
    return _device_classify(ref_cluster, n_clusters, ptr, nbr, w, weight_frac, min_degree, min_weight)


def _gpu_levels(options):
    from nabo_amd._paths import _DeviceGraph
    graphs = []

    def make(n, ptr, nbr):
        g = _DeviceGraph(ptr, nbr, 0, options)
        graphs.append(g)
        return lambda seeds, k: g.set_levels([0, len(seeds)], seeds, k)[0]
    return make, graphs


@pytest.mark.gpu
@pytest.mark.parametrize("options", OPTIONS)
def test_fixture_parity(gpu_lib, golden, options):
    make, graphs = _gpu_levels(options)
    try:
        assert cref.check_fixtures(golden("paths"), golden("classify"), _gpu_classify, make) >= 150
    finally:
        for g in graphs:
            g.close()


@pytest.mark.gpu
def test_quirks_match_reference(gpu_lib, golden):
    for options in OPTIONS:
        make, graphs = _gpu_levels(options)
        try:
            assert cref.check_quirks(golden("classify"), _gpu_classify, make) >= 250
        finally:
            for g in graphs:
                g.close()


@pytest.mark.gpu
def test_file_level_functions_both_layouts(gpu_lib):
    py = _interpreter()
    if py is None:
        pytest.skip("no interpreter with h5py in this image")
    r = subprocess.run([py, os.path.join(HERE, "_classify_case.py")], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       universal_newlines=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][len("RESULT "):])
    assert res["checked"] >= 60 and res["differ"] == [], res


def _bit_equal(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.int64), np.asarray(b, dtype=np.float64).view(np.int64))


@pytest.mark.gpu
def test_scale_200k_snn_graph_against_restatement(gpu_lib):
    import nabo_amd
    from nabo_amd._mapping import snn_edges
    from nabo_amd._synth import pca_like
    n, k, ncl = 200000, 11, 32
    ref = pca_like(n, 30, seed=41)
    r_idx, _ = nabo_amd.knn(ref, ref, k, metric=nabo_amd.EUCLIDEAN, drop_first=True)
    tgt = pca_like(n, 30, seed=43)
    t_idx, _ = nabo_amd.knn(tgt, ref, k, metric=nabo_amd.EUCLIDEAN)
    tt, tj, tw = snn_edges(t_idx, r_idx, k)
    order = np.argsort(tt, kind="stable")
    ptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(tt, minlength=n), out=ptr[1:])
    nbr, w = tj[order].astype(np.int64), np.asarray(tw, dtype=np.float64)[order]
    rng = np.random.default_rng(9)
    rc = rng.integers(0, ncl, n).astype(np.int32)
    rc[rng.random(n) < 0.1] = -1                               # reference nodes without a cluster
    for wf, md, mw in ((0.5, 2, 0.1), (0.3, 3, 0.0)):
        got = nabo_amd.classify_from_edges(rc, ptr, nbr, w, wf, md, mw, n_clusters=ncl)
        lab, best, tot, cnt, _ = cref.classify(rc, ncl, ptr, nbr, w, wf, md, mw, details=True)
        assert np.array_equal(got["label"], lab), (wf, md, mw)
        assert _bit_equal(got["best"], best) and _bit_equal(got["total"], tot), (wf, md, mw)
        assert np.array_equal(got["counts"], cnt) and int(cnt.sum()) == n
        assert (lab >= 0).sum() > 0 and (lab < 0).sum() > 0


@pytest.mark.gpu
def test_synthetic_rows(gpu_lib):
    """rows of length 0, 1, ~300 with repeats, a row longer than the kernel's stage, every weight below min_weight"""
    import nabo_amd
    rng = np.random.default_rng(4)
    n_ref, ncl = 500, 7
    rc = rng.integers(-1, ncl, n_ref).astype(np.int32)
    lens = [0, 1, 300, 0, 15, 1500, 2, 310, 1, 0] + rng.integers(0, 40, 200).tolist() + [1100, 3]
    rows = [rng.integers(0, n_ref if ln > 400 else 120, ln) for ln in lens]     # 300 draws from 120 nodes: many repeats
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    nbr = np.concatenate(rows).astype(np.int64)
    w = rng.choice([0.05, 0.11, 0.25, 0.33, 1.0, 0.1], nbr.shape[0])
    w[ptr[4]:ptr[5]] = 0.05                                   # a row whose weights are all below min_weight
    for wf, md, mw in ((0.5, 2, 0.1), (0.05, 1, 0.1), (0.0, 0, -1.0), (0.5, 2, 5.0)):
        got = nabo_amd.classify_from_edges(rc, ptr, nbr, w, wf, md, mw, n_clusters=ncl)
        lab, best, tot, cnt, _ = cref.classify(rc, ncl, ptr, nbr, w, wf, md, mw, details=True)
        assert np.array_equal(got["label"], lab), (wf, md, mw, np.nonzero(got["label"] != lab)[0][:5])
        assert _bit_equal(got["best"], best) and _bit_equal(got["total"], tot), (wf, md, mw)
        assert np.array_equal(got["counts"], cnt)
    # more clusters than the counting kernel's LDS histogram holds, and no optional outputs
    rc2 = rng.integers(0, 3000, n_ref).astype(np.int32)
    got = nabo_amd.classify_from_edges(rc2, ptr, nbr, w, 0.2, 1, 0.0, n_clusters=3000)
    lab, cnt = cref.classify(rc2, 3000, ptr, nbr, w, 0.2, 1, 0.0)
    assert np.array_equal(got["label"], lab) and np.array_equal(got["counts"], cnt)


def _few(rng, n):
    return rng.integers(0, 12, n).tolist()


def _stage_cases():
    """name -> rows as (length, pool) pairs: the row's neighbours are `length` draws from the first `pool` reference
    nodes, all distinct when pool is None.  The kernel stages 64 rows at a time in pieces of at most 1 024 edges cut at
    row boundaries; a single row of more than 1 024 edges is walked in the device scratch."""
    rng = np.random.default_rng(21)
    short = lambda lens: [(int(ln), 120) for ln in lens]
    return {
        # the last row length staged in LDS and the first that takes the scratch, each between short rows
        "rows_of_1023_1024_1025": short([5]) + [(1023, None)] + short([0]) + [(1024, None)] + short([3]) + [(1025, None)] + short([2]),
        # the longest row the ABI accepts, the first loop's repeat search never cut short
        "row_of_4096_distinct": short([3]) + [(4096, None)] + short([7]),
        # the same length with every neighbour repeated about twenty times
        "row_of_4096_from_200_nodes": short([2, 0]) + [(4096, 200)] + short([9]),
        # two scratch rows in a row: `done` advances by one twice, the empty rows before and after join the next stage
        "two_long_rows_between_empty_ones": short([4, 0]) + [(1100, 3000), (1300, 3000)] + short([0, 6]),
        # a whole batch is exactly one stage: one pass, run = 64
        "64_rows_of_16": [(16, 300)] * 64,
        # one edge more: the stage is cut after row 62, row 63 is a stage of its own
        "64_rows_of_16_one_of_17": [(16, 300)] * 40 + [(17, 300)] + [(16, 300)] * 23,
        # a scratch row in lane 63 of batch 0, in lane 0 of batch 1 and as the last row of a final batch of 3 rows
        "long_rows_in_lane_0_and_63_and_last": short(_few(rng, 63)) + [(1200, 3000), (1500, 3000)] + short(_few(rng, 63)) + short([4, 0])
                                               + [(1026, 3000)],
        # a batch of one lane, a full batch, a full batch and a final batch of one row
        "n_targets_1": [(30, 120)],
        "n_targets_64": short(rng.integers(0, 40, 64)),
        "n_targets_65": short(rng.integers(0, 40, 65)),
    }


@pytest.mark.gpu
@pytest.mark.parametrize("wf,md,mw", [(0.5, 2, 0.1), (0.05, 1, 0.1), (0.0, 0, -1.0), (0.5, 2, 5.0)])
@pytest.mark.parametrize("name", sorted(_stage_cases()))
def test_rows_at_the_stage_boundaries(gpu_lib, name, wf, md, mw):
    """every case of _stage_cases (the comments there say which branch of classify_rows_kernel each one is the first to
    run) with each of the four settings of test_synthetic_rows: labels and counts equal to the restatement, best and total
    bit for bit.  Two rows of 4 096 edges in all, and a call for each setting: one lane walks such a row with O(len^2)
    reads, more than a second for the row without repeats."""
    import nabo_amd
    rows_of = _stage_cases()[name]
    rng = np.random.default_rng(len(name) + len(rows_of))
    n_ref, ncl = 5000, 7
    rc = rng.integers(-1, ncl, n_ref).astype(np.int32)
    rows = [rng.permutation(n_ref)[:ln] if pool is None else rng.integers(0, pool, ln) for ln, pool in rows_of]
    lens = [len(r) for r in rows]
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    nbr = np.concatenate(rows).astype(np.int64)
    w = rng.choice([0.05, 0.11, 0.25, 0.33, 1.0, 0.1], nbr.shape[0])
    # what the names promise
    if name == "64_rows_of_16":
        assert len(lens) == 64 and ptr[-1] == 1024
    if name == "64_rows_of_16_one_of_17":
        assert len(lens) == 64 and ptr[-1] == 1025 and ptr[63] <= 1024
    if name == "long_rows_in_lane_0_and_63_and_last":
        assert len(lens) == 131 and min(lens[63], lens[64], lens[130]) > 1024 and max(lens[:63] + lens[65:130]) < 12
    if name.startswith("row_of_4096"):
        assert max(lens) == 4096
        assert len(set(rows[lens.index(4096)].tolist())) == (4096 if "distinct" in name else 200)
    if name.startswith("n_targets"):
        assert len(lens) == int(name.split("_")[-1])
    got = nabo_amd.classify_from_edges(rc, ptr, nbr, w, wf, md, mw, n_clusters=ncl)
    lab, best, tot, cnt, _ = cref.classify(rc, ncl, ptr, nbr, w, wf, md, mw, details=True)
    assert np.array_equal(got["label"], lab), np.nonzero(got["label"] != lab)[0][:5]
    assert _bit_equal(got["best"], best) and _bit_equal(got["total"], tot)
    assert np.array_equal(got["counts"], cnt) and int(cnt.sum()) == len(lens)
    if (wf, md, mw) == (0.05, 1, 0.1):
        assert (lab >= 0).any()


def _sets(n, n_sets, rng):
    sets = [rng.integers(0, n, int(rng.integers(1, 9))).tolist() for _ in range(n_sets)]
    sets[0] = [0]
    if n_sets > 2:
        sets[1] = sets[0] + sets[2]                            # overlapping sets
        sets[2] = sets[2] + sets[2][:1] * 3                    # repeated members
    if n_sets > 5:
        sets[5] = []                                           # an empty set
    if n_sets > 7:
        sets[7] = rng.integers(0, n, 200).tolist()             # more than 64 seeds under one bit
    return sets


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(_graphs()))
def test_set_levels_against_bfs(gpu_lib, name):
    from nabo_amd._paths import _DeviceGraph
    n, arcs = _graphs()[name]
    ptr, nbr = _csr(n, arcs)
    uptr, ucol = orc.undirected(n, ptr, nbr)
    rng = np.random.default_rng(13)
    for options in OPTIONS:
        g = _DeviceGraph(ptr, nbr, 0, options)
        try:
            for n_sets in (1, 64, 65, 130):
                sets = _sets(n, n_sets, rng)
                sp = np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.int64)
                mem = np.array([v for s in sets for v in s], dtype=np.int64)
                for max_level in (0, 2, -1):
                    if max_level < 0 and n_sets == 130 and options is not None:
                        continue                               # the unlimited 130-set sweep once per graph is enough
                    got = g.set_levels(sp, mem, max_level)
                    want = np.stack([_bfs_levels(uptr, ucol, s, max_level) for s in sets])
                    assert np.array_equal(got, want), (name, options, n_sets, max_level)
            # the group-hops state is intact after set sweeps, and the other way round
            s, u = g.group_hops([0, 2], [0, n - 1])
            d = int(orc.bfs(uptr, ucol, 0, [n - 1])[n - 1])
            assert (int(s[0]), int(u[0])) == ((d, 0) if d >= 0 else (0, 1))
            assert np.array_equal(g.set_levels([0, 1], [0], -1)[0], _bfs_levels(uptr, ucol, [0], -1))
        finally:
            g.close()


@pytest.mark.gpu
def test_bad_sets_are_refused_on_a_resident_graph(gpu_lib):
    """members out of range or negative, a non-monotone set_ptr, set_ptr[0] != 0 and a NULL out_level are refused by
    the library itself (the Python wrapper's own checks are bypassed), and the graph's state is untouched"""
    from nabo_amd import _lib
    from nabo_amd._paths import _DeviceGraph
    n = 50
    ptr, nbr = _csr(n, [(i, i + 1) for i in range(n - 1)])
    uptr, ucol = orc.undirected(n, ptr, nbr)
    L = _lib.lib()
    g = _DeviceGraph(ptr, nbr, 0)
    try:
        out = np.full((2, n), 7, dtype=np.int32)

        def raw(set_ptr, members, out_ptr):
            sp, mem = np.array(set_ptr, dtype=np.int64), np.array(members, dtype=np.int64)
            return L.nabo_refgraph_set_levels(g._h, len(set_ptr) - 1, sp.ctypes.data, mem.ctypes.data, -1, out_ptr)

        for set_ptr, members in (([0, 1], [n]), ([0, 1], [-1]), ([0, 2, 3], [0, 1, n + 5]), ([0, 2, 1], [0, 1]), ([1, 2], [0, 1])):
            assert raw(set_ptr, members, out.ctypes.data) == _lib.E_INVALID, (set_ptr, members)
        assert raw([0, 1], [3], None) == _lib.E_INVALID and b"out_level" in L.nabo_last_error()
        assert (out == 7).all()                                 # nothing was written
        with pytest.raises(ValueError):
            g.set_levels([0, 1], [n])                           # through the wrapper: ValueError
        # a valid call after the refusals is still right, and so is group_hops
        got = g.set_levels([0, 2, 3], [0, 0, n - 1], -1)
        assert np.array_equal(got, np.stack([_bfs_levels(uptr, ucol, [0], -1), _bfs_levels(uptr, ucol, [n - 1], -1)]))
        s_, u_ = g.group_hops([0, 2], [0, n - 1])
        assert (int(s_[0]), int(u_[0])) == (n - 1, 0)
    finally:
        g.close()


def _bfs_levels(uptr, ucol, members, max_level):
    """levels of one set from the tests' single-source BFS: the minimum over its distinct members"""
    n = uptr.shape[0] - 1
    best = np.full(n, -1, dtype=np.int64)
    for s in sorted(set(members)):
        d = orc.bfs(uptr, ucol, s)
        best = np.where((d >= 0) & ((best < 0) | (d < best)), d, best)
    if max_level >= 0:
        best[best > max_level] = -1
    return best.astype(np.int32)


@pytest.mark.gpu
def test_plain_c_consumer_gets_the_quirk_answers(gpu_lib, golden, tmp_path):
    from nabo_amd._classify import _cluster_ids
    exe = build_cluster_check(tmp_path)
    case, ref, pos, _, _, targets = cref.quirk_graph(golden("classify"))
    cd = [c["kwargs"]["cluster_dict"] for c in case["calls"] if c["kwargs"].get("cluster_dict")][0]
    labels, rc = _cluster_ids(ref, pos, len(ref), cd)
    _, tp, tn, tw = targets["T"]
    text = "%d %d %d 0.5 2 0.1\n" % (len(ref), len(labels), len(tp) - 1)
    text += " ".join(str(int(x)) for x in rc) + "\n" + " ".join(str(int(x)) for x in tp) + "\n"
    text += "\n".join("%d %r" % (int(a), float(b)) for a, b in zip(tn, tw)) + "\n"
    r = subprocess.run([exe, "run"], input=text, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
    assert r.returncode == 0, r.stdout
    lab, best, tot, cnt, _ = cref.classify(rc, len(labels), tp, tn, tw, 0.5, 2, 0.1, details=True)
    rows = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("row ")]
    assert [int(x[2]) for x in rows] == lab.tolist()
    assert _bit_equal([float(x[3]) for x in rows], best) and _bit_equal([float(x[4]) for x in rows], tot)
    assert [int(ln.split()[2]) for ln in r.stdout.splitlines() if ln.startswith("count ")] == cnt.tolist()
    # and they are the reference's: the recorded default call with this cluster_dict
    want = [c for c in case["calls"] if c["method"] == "classify_target" and c["kwargs"] == {"target": "T", "cluster_dict": cd}][0]
    assert [labels[i] if i >= 0 else "NA" for i in lab.tolist()] == list(want["result"][1].values())
