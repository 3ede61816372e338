"""The UMAP transform (include/nabo_umap_transform.h, nabo_amd/_umap.py) without a GPU: the C header and its symbols, the
tests' numpy restatement (tests/_umap_transform_ref.py) against a scalar loop written from the definition, the condition
that no list case sits on a threshold of the sigma search, the whole-run golden reproduced for one seed, argument checks,
the no-device failure, and the frame `make_target_umap` returns with the device step stubbed."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import nabo_amd
from nabo_amd import _lib, _umap

import _umap_ref as ur
import _umap_transform_ref as tr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = tr.list_cases()
AB = (1.5769436135065888, 0.8950607193577038)


def test_public_names_and_symbols():
    for n in ("make_target_umap", "umap_transform", "UmapTransform"):
        assert n in nabo_amd.__all__ and callable(getattr(nabo_amd, n))
    src = open(os.path.join(REPO, "include", "nabo_umap_transform.h")).read()
    assert '#include "nabo_knn.h"' in src
    for other in ("nabo_knn.h", "nabo_umap.h"):
        assert "nabo_umap_transform" not in open(os.path.join(REPO, "include", other)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert sorted(set(re.findall(r"\b(nabo_[a-z0-9_]+)\s*\(", src))) == sorted(_lib.UMAP_TRANSFORM_SYMBOLS)
    others = (_lib.SYMBOLS + _lib.GRAPH_SYMBOLS + _lib.CLUSTER_SYMBOLS + _lib.DE_SYMBOLS + _lib.PCA_SYMBOLS + _lib.PCA_FIT_SYMBOLS
              + _lib.QC_SYMBOLS + _lib.LAYOUT_SYMBOLS + _lib.UMAP_SYMBOLS + _lib.COMMUNITY_SYMBOLS + _lib.POTENTIAL_SYMBOLS)
    assert not set(_lib.UMAP_TRANSFORM_SYMBOLS) & set(others)
    L = _lib.lib()
    for n in _lib.UMAP_TRANSFORM_SYMBOLS:
        assert hasattr(L, n), n
    group = _umap.transform_geometry()
    assert group in (1, 2, 4, 8, 16, 32, 64)
    hip = open(os.path.join(REPO, "nabo_amd", "csrc", "umap_transform.hip")).read()
    assert "UT_GROUP = %d;" % group in hip
    # the helpers the two UMAP steps share are defined once
    fit = open(os.path.join(REPO, "nabo_amd", "csrc", "umap.hip")).read()
    common = open(os.path.join(REPO, "nabo_amd", "csrc", "umap_common.h")).read()
    for name in ("umap_mix(uint64_t z)", "umap_tree(double v)", "umap_clip(double v)"):
        assert name in common and name not in fit and name not in hip


def test_header_is_plain_c_and_links(tmp_path):
    _lib.lib()
    exe = os.path.join(str(tmp_path), "umap_transform_check")
    cmd = ["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(REPO, "include"),
           os.path.join(REPO, "tests", "abi_c", "umap_transform_check.c"), "-L" + os.path.join(REPO, "nabo_amd"), "-lnabo_knn",
           "-Wl,-rpath," + os.path.join(REPO, "nabo_amd"), "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0 and "%d entry points" % len(_lib.UMAP_TRANSFORM_SYMBOLS) in r.stdout, r.stdout


@pytest.mark.parametrize("name", list(CASES))
def test_no_list_case_sits_on_a_threshold(golden, name):
    """a condition on the cases, so that the GPU test may demand bit-equal sigma everywhere: a flagged row means another
    seed is to be chosen, not that the row is excused"""
    c = CASES[name]
    g = tr.graph(c["idx"], c["dist"], c["Y"])
    assert not g["flagged"].any()
    assert int(golden("umap_transform")["list_flagged"]) == 0
    m, k = c["idx"].shape
    assert k in (2, 5, 15, 17, 56) + tr.GROUP_K and m in (1, 17, 333)
    if name == "k%d_m17" % k and k in tr.GROUP_K:
        # the width of the graph kernel and the arcs a lane of the run kernel holds, as the launchers choose them
        width, arcs = (8 if k <= 8 else 16 if k <= 16 else 32 if k <= 32 else 64), -(-k // _umap.transform_geometry())
        assert (k, width, arcs) in ((8, 8, 1), (9, 16, 1), (16, 16, 1), (32, 32, 2), (33, 64, 3), (48, 64, 3)) and len(c["Y"]) == 200
    # the search met its target wherever the floor did not act and the row is not all zeros
    ok = np.abs(g["psum_at"] - math.log2(k)) < 1e-5
    assert ok[~g["floored"] & (c["dist"][:, -1] > 0) & (k > 2)].all()
    assert ((g["memb"] > 0) & (g["memb"] <= 1)).all() and np.isfinite(g["y0"]).all()
    # the start is a convex combination of the neighbours' positions, up to rounding
    nb = c["Y"][c["idx"]]
    assert (g["y0"] >= nb.min(axis=1) - 1e-12).all() and (g["y0"] <= nb.max(axis=1) + 1e-12).all()
    if name == "k15_m333":
        assert c["dist"][3, 0] == 0 and c["idx"][3, 0] == 7 and g["memb"][3, 0] == 1
    if name == "zeros_k5_m17":
        assert (c["dist"][2] == 0).all() and (g["memb"][2] == 1).all() and 0 < g["sigma"][2] < 1e-15
        assert (c["dist"][5, :2] == 0).all() and c["dist"][5, 2] > 0
    if name == "ties_k5_m17":
        assert c["dist"][9, 1] == c["dist"][9, 2] == c["dist"][9, 3]
    if name == "k48_m17":
        assert c["dist"][4, 0] == 0 and c["idx"][4, 0] == 9 and g["memb"][4, 0] == 1 and c["dist"][4, 1] > 0


def scalar_graph(idx, dist, Y):
    """parts B', C' and the start of the header, row by row in Python floats"""
    out = []
    for row_i, row_d in zip(idx.tolist(), dist.tolist()):
        k = len(row_d)
        target = math.log2(k)
        tree = lambda v: float(tr.tree_sum(np.array(v)))
        lo, hi, mid = 0.0, math.inf, 1.0
        for _ in range(64):
            p = tree([0.0] + [1.0 if d <= 0 else math.exp(-(d / mid)) for d in row_d[1:]])
            if abs(p - target) < 1e-5:
                break
            if p > target:
                hi = mid
                mid = (lo + hi) / 2.0
            else:
                lo = mid
                mid = mid * 2.0 if math.isinf(hi) else (lo + hi) / 2.0
        sigma = max(mid, 1e-3 * (tree(row_d) / k))
        a = [1.0 if d <= 0 or sigma == 0 else math.exp(-(d / sigma)) for d in row_d]
        s = tree(a)
        y = [0.0] * Y.shape[1]
        for t in range(k):
            for c in range(Y.shape[1]):
                y[c] = y[c] + (a[t] / s) * float(Y[row_i[t], c])
        out.append((sigma, a, y))
    return out


@pytest.mark.parametrize("name", ["k5_m1", "k17_m17", "zeros_k5_m17", "ties_k5_m17", "k2_m17"])
def test_restated_graph_against_a_scalar_loop(name):
    c = CASES[name]
    g = tr.graph(c["idx"], c["dist"], c["Y"])
    want = scalar_graph(c["idx"], c["dist"], c["Y"])
    assert [w[0] for w in want] == g["sigma"].tolist()
    np.testing.assert_allclose(g["memb"], np.array([w[1] for w in want]), rtol=0, atol=tr.MEMB_TOL)   # numpy's exp, math's exp
    bound = tr.start_bound(c["idx"], g["memb"], c["Y"])
    assert (np.abs(g["y0"] - np.array([w[2] for w in want])) <= bound).all() and bound.max() < 1e-12


def scalar_epoch(ep, y, t, next_, nneg):
    """one epoch from the header's part D', target by target, arc by arc and sample by sample in Python floats and
    integers; returns the new positions, the counts and the schedule after it"""
    dims, G, k = len(y[0]), ep.group, ep.k
    alpha = 0.25 * (1.0 - float(t) / float(ep.n_epochs))
    clip = lambda v: 4.0 if v > 4.0 else -4.0 if v < -4.0 else v
    out, counts = [], []
    next_, nneg = [list(r) for r in next_], [list(r) for r in nneg]
    for i in range(ep.m):
        lanes = [[0.0] * dims for _ in range(G)]
        na = nn = ks = 0
        for tp in range(k):
            lane = lanes[tp % G]
            if not (ep.memb[i, tp] >= 1.0 / ep.n_epochs and next_[i][tp] <= t):
                continue
            eps = 1.0 / float(ep.memb[i, tp])
            epn = eps / ep.nsr
            j = int(ep.idx[i, tp])
            D = [y[i][c] - float(ep.Y[j, c]) for c in range(dims)]
            d2 = sum(x * x for x in D)
            c = (ep.ca * d2 ** (ep.b - 1.0)) / (ep.a * d2 ** ep.b + 1.0) if d2 > 0 else 0.0
            for x in range(dims):
                lane[x] += clip(c * D[x])
            na += 1
            next_[i][tp] += eps
            ms = int((t - nneg[i][tp]) / epn)
            for p in range(ms):
                kk = ur.sample(ep.seed, t, (ep.first_row + i) * k + tp, p, ep.n_ref)
                nn += 1
                ks = (ks + kk) & ur.M64
                D = [y[i][c] - float(ep.Y[kk, c]) for c in range(dims)]
                d2 = sum(x * x for x in D)
                c = ep.cr / ((0.001 + d2) * (ep.a * d2 ** ep.b + 1.0)) if d2 > 0 else 0.0
                for x in range(dims):
                    lane[x] += clip(c * D[x])
            nneg[i][tp] += ms * epn
        S = [float(ur.tree_sum(np.array([lanes[l][x] for l in range(G)]))) for x in range(dims)]
        out.append([y[i][x] + alpha * S[x] for x in range(dims)])
        counts.append((na, nn, ks))
    return out, counts, next_, nneg


@pytest.mark.parametrize("name,nsr,group,first_row", [("k17_m17", 5, 16, 0), ("k2_m17", 1, 16, 1000), ("k56_m17", 5, 16, 7),
                                                      ("k17_m17", 2, 4, 3)])
def test_restated_epoch_against_a_scalar_loop(name, nsr, group, first_row):
    """the vectorised restatement takes every decision of the scalar loop (which arcs fire, how many samples, which
    reference cells they name) and lands within rounding of its positions (numpy's vectorised pow may differ from
    Python's)"""
    c = CASES[name]
    g = tr.graph(c["idx"], c["dist"], c["Y"])
    n_ep = 20                                                  # 1 / 20 lies above the smallest membership of k56_m17
    ep = tr.Epochs(c["idx"], g["memb"], c["Y"], first_row, n_ep, nsr, 1.0, AB[0], AB[1], 5, group)
    y = g["y0"].copy()
    y[1] = c["Y"][c["idx"][1, 0]]                              # on top of a neighbour: d2 == 0
    fired = drawn = 0
    for t in range(n_ep):
        nx, ng = ep.next.copy(), ep.nneg.copy()
        o = ep.step(y)
        want, counts, nx2, ng2 = scalar_epoch(ep, y.tolist(), t, nx.tolist(), ng.tolist())
        assert [q[0] for q in counts] == o["n_attr"].tolist() and [q[1] for q in counts] == o["n_neg"].tolist()
        assert [q[2] for q in counts] == [int(v) for v in o["idx_sum"]]
        assert nx2 == ep.next.tolist() and ng2 == ep.nneg.tolist()
        np.testing.assert_allclose(o["y"], np.array(want), rtol=0, atol=1e-12)
        if t == 0:
            assert o["n_attr"].sum() == 0                      # next = eps >= 1 > 0
        fired += int(o["n_attr"].sum())
        drawn += int(o["n_neg"].sum())
        y = o["y"]
    assert fired > 100 and drawn >= fired * min(nsr, 2) // 2 and np.isfinite(y).all()
    if name == "k56_m17":
        assert not ep.live.all(), "some arc was meant to lie below 1 / n_epochs"
        assert np.isinf(ep.next[~ep.live]).all()


def test_schedule_and_batches():
    """a live arc fires about n_epochs a times; the samples of a row depend on its global number, not on the batch"""
    c = CASES["k15_m333"]
    g = tr.graph(c["idx"], c["dist"], c["Y"])
    ep = tr.Epochs(c["idx"], g["memb"], c["Y"], 0, 100, 5, 1.0, AB[0], AB[1], 0, 16)
    fires = np.zeros(g["memb"].shape, dtype=np.int64)
    for _ in range(100):
        i, tp, ms = ep.firing()
        assert (ms >= 0).all()
        fires[i, tp] += 1
    want = np.floor(99.0 * g["memb"] + 1e-9)
    assert (np.abs(fires - want)[ep.live] <= 1).all() and (fires[~ep.live] == 0).all() and fires[g["memb"] == 1].min() == 99
    part = tr.Epochs(c["idx"][100:], g["memb"][100:], c["Y"], 100, 100, 5, 1.0, AB[0], AB[1], 0, 16)
    i = np.arange(5)
    assert np.array_equal(part.samples(7, i, i + 2, 1), ep.samples(7, i + 100, i + 2, 1))
    assert part.samples(7, i, i + 2, 1).tolist() == [ur.sample(0, 7, (100 + int(x)) * 15 + int(x) + 2, 1, 600) for x in i]


def test_whole_run_golden_is_reproduced(golden):
    gold = golden("umap_transform")
    X, grp = ur.blobs()
    ref, tgt = tr.held_out()
    assert np.array_equal(ref, gold["ref_rows"]) and np.array_equal(tgt, gold["target_rows"])
    assert len(tgt) == 60 and (np.bincount(grp[tgt]) == 10).all() and int(gold["group"]) == _umap.transform_geometry()
    a, b = gold["ab"]
    assert (a, b) == _umap.find_ab_params(1.0, 0.1)
    y0, y = tr.run(X[tgt], X[ref], gold["ref_Y2"], int(gold["whole_k"]), int(gold["whole_epochs"]), a, b, 0, int(gold["group"]))
    s, ie = tr.target_share(y, gold["ref_Y2"], X[tgt], X[ref])
    np.testing.assert_allclose(y, gold["whole_y_seed0_dims2"], rtol=0, atol=1e-6)
    assert abs(s - gold["share"][0, 0]) <= 1.0 / 600 and (grp[ref][ie] == grp[tgt][:, None]).all()
    assert gold["same_group"].all() and gold["share"].shape == (2, 8)
    assert (np.abs(y - y0).max(axis=1) > 0).all()


GOOD = dict(Z=np.random.default_rng(1).normal(size=(7, 4)), X_ref=np.random.default_rng(2).normal(size=(30, 4)),
            ref_embedding=np.random.default_rng(3).uniform(0, 10, size=(30, 2)), n_neighbors=5, n_epochs=10)


@pytest.mark.parametrize("change", [
    {"Z": np.zeros(7)},                                      # not 2-D
    {"Z": np.full((7, 4), np.nan)},
    {"Z": np.zeros((0, 4))},                                 # no target
    {"Z": np.zeros((7, 3))},                                 # other components than the reference
    {"X_ref": np.zeros((1, 4))},                             # too few reference cells
    {"X_ref": np.full((30, 4), np.inf)},
    {"ref_embedding": np.zeros((29, 2))},                    # another row count than X_ref
    {"ref_embedding": np.zeros((30, 4))},                    # four dimensions
    {"ref_embedding": np.full((30, 2), np.nan)},
    {"ref_embedding": "frame"},
    {"n_neighbors": 1},
    {"n_neighbors": 57},                                     # above NABO_MAX_K
    {"n_neighbors": 31},                                     # above n_ref
    {"n_neighbors": 5.5},
    {"n_epochs": 0},
    {"negative_sample_rate": 0},
    {"repulsion_strength": np.inf},
    {"spread": 0.0},
    {"min_dist": -0.1},
    {"a": 1.5},                                              # a without b
    {"a": -1.0, "b": 1.0},
    {"seed": -1},
    {"batch": 0},
    {"batch": 2.5},
])
def test_bad_arguments_raise_before_any_device(change, monkeypatch):
    def no_library(*a, **k):
        raise AssertionError("the library was called before the arguments were checked")
    monkeypatch.setattr(_lib, "lib", no_library)
    with pytest.raises(ValueError) as e:
        nabo_amd.umap_transform(**dict(GOOD, **change))
    assert str(e.value).startswith("ERROR: ")


@pytest.mark.parametrize("what,change", [
    ("set_knn", {"idx": np.zeros((4, 3, 1), dtype=np.int64)}),
    ("set_knn", {"val": np.zeros((4, 4))}),                  # another shape than idx
    ("set_knn", {"idx": np.tile(np.arange(3), (4, 1)) + 10}),   # no such reference cell
    ("set_knn", {"val": np.tile(np.array([0.0, 2.0, 1.0]), (4, 1))}),   # not ascending
    ("set_knn", {"val": np.tile(np.array([0.0, 1.0, np.nan]), (4, 1))}),
    ("set_knn", {"val": np.tile(np.array([-1.0, 1.0, 2.0]), (4, 1))}),
    ("set_graph", {"val": np.tile(np.array([0.5, 1.5, 0.1]), (4, 1))}),   # a membership above 1
    ("set_graph", {"val": np.tile(np.array([0.5, -0.5, 0.1]), (4, 1))}),
    ("set_graph", {"val": np.tile(np.array([0.5, np.nan, 0.1]), (4, 1))}),
])
def test_bad_lists_raise_before_any_device(what, change):
    good = dict(idx=np.tile(np.arange(3), (4, 1)), val=np.tile(np.array([0.0, 1.0, 2.0]) / (3 if what == "set_graph" else 1), (4, 1)))
    args = dict(good, **change)
    with pytest.raises(ValueError) as e:
        _umap._check_target_lists(args["idx"], args["val"], 10, memberships=what == "set_graph")
    assert str(e.value).startswith("ERROR: ")
    _umap._check_target_lists(good["idx"], good["val"], 10, memberships=what == "set_graph")
    # a list of more entries than there are reference cells
    with pytest.raises(ValueError):
        _umap._check_target_lists(good["idx"], good["val"], 2)


def test_default_epochs():
    assert _umap.default_transform_epochs(10000) == 100 and _umap.default_transform_epochs(10001) == 30


def test_no_device_is_a_loud_failure():
    if nabo_amd.device_count() > 0:
        pytest.skip("a GPU is visible here; the no-device path is covered on the CPU box")
    with pytest.raises(nabo_amd.NaboError) as e:
        nabo_amd.umap_transform(**GOOD)
    assert "no HIP device" in str(e.value)


def test_make_target_umap_returns_the_reference_frame(monkeypatch):
    pd = pytest.importorskip("pandas")
    ref_cells = ["R%02d-1" % i for i in range(6)]
    cells = ["AAAC-1", "AAAG-1", "AATT-1", "ACGT-1"]
    Xr, Z = np.arange(30.0).reshape(6, 5), np.arange(20.0).reshape(4, 5) + 0.5
    seen = {"read": []}

    def read_cells(fn, grp, use_comps):
        seen["read"].append((fn, grp, use_comps))
        return (ref_cells, Xr[:, :use_comps]) if fn == "ref.h5" else (cells, Z[:, :use_comps])

    def transform(Zt, X_ref, Y, n_neighbors, n_epochs, spread, min_dist, repulsion_strength, negative_sample_rate, seed, device=0,
                  batch=None):
        seen["call"] = dict(Z=Zt, X_ref=X_ref, Y=Y, n_neighbors=n_neighbors, n_epochs=n_epochs, spread=spread, min_dist=min_dist,
                            repulsion_strength=repulsion_strength, negative_sample_rate=negative_sample_rate, seed=seed, device=device,
                            batch=batch)
        return np.arange(len(Zt) * Y.shape[1], dtype=np.float64).reshape(len(Zt), Y.shape[1])

    monkeypatch.setattr(_umap, "_read_cells", read_cells)
    monkeypatch.setattr(_umap, "umap_transform", transform)
    ref_umap = pd.DataFrame(np.arange(12.0).reshape(6, 2) * 0.25, index=[c + "_REF" for c in ref_cells], columns=["Dim1", "Dim2"])
    df = nabo_amd.make_target_umap("ref.h5", "tgt.h5", ref_umap, 3, 15, 1.0, 2.0, 0.1, 50, data_group="other", index_suffix="_KO",
                                   verbose=False, seed=4, batch=2)
    assert isinstance(df, pd.DataFrame) and df.shape == (4, 2)
    assert list(df.index) == [c + "_KO" for c in cells] and list(df.columns) == list(ref_umap.columns)
    assert np.array_equal(df.values, np.arange(8.0).reshape(4, 2))
    assert seen["read"] == [("ref.h5", "data", 3), ("tgt.h5", "other", 3)]
    f = seen["call"]
    assert f["Z"].shape == (4, 3) and f["X_ref"].shape == (6, 3) and np.array_equal(f["Y"], ref_umap.values)
    assert (f["n_neighbors"], f["n_epochs"], f["spread"], f["min_dist"], f["repulsion_strength"]) == (15, 50, 1.0, 0.1, 2.0)
    assert (f["negative_sample_rate"], f["seed"], f["device"], f["batch"]) == (5, 4, 0, 2)
    with pytest.raises(ValueError) as e:                     # a frame of another reference
        nabo_amd.make_target_umap("ref.h5", "tgt.h5", ref_umap.iloc[:5], 3, 15, verbose=False)
    assert str(e.value).startswith("ERROR: ") and "5 rows" in str(e.value)
    with pytest.raises(ValueError):
        nabo_amd.make_target_umap("ref.h5", "tgt.h5", np.zeros((6, 2)), 3, 15, verbose=False)
    with pytest.raises(TypeError):
        nabo_amd.make_target_umap("ref.h5", "tgt.h5", ref_umap, 3, 15, 1.0, 2.0, 0.1, 50, "data", "", False, 4)   # seed is keyword-only
