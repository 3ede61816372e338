"""The UMAP step (include/nabo_umap.h, nabo_amd/_umap.py) without a GPU: the C header and its symbols, the invariants of
the tests' numpy restatement (tests/_umap_ref.py) and its agreement with a scalar loop written from the definition, the
schedule's decisions and the negative samples reproduced one at a time, the a, b fit against scipy's, the start
positions, argument checks, the no-device failure, and the frame `make_umap` returns with the device step stubbed."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import nabo_amd
from nabo_amd import _lib, _umap

import _umap_ref as ur

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ur.graph_cases()
N_EPOCHS = (ur.N_EPOCHS_PRUNING, ur.N_EPOCHS_KEEPING)


@pytest.fixture(scope="module")
def gold(golden):
    return golden("umap")


def test_public_names_and_symbols():
    for n in ("make_umap", "umap_fit", "umap_fuzzy_graph", "find_ab_params", "Umap"):
        assert n in nabo_amd.__all__ and callable(getattr(nabo_amd, n))
    src = open(os.path.join(REPO, "include", "nabo_umap.h")).read()
    assert '#include "nabo_knn.h"' in src and "nabo_umap.h" not in open(os.path.join(REPO, "include", "nabo_knn.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert sorted(set(re.findall(r"\b(nabo_[a-z0-9_]+)\s*\(", src))) == sorted(_lib.UMAP_SYMBOLS)
    others = (_lib.SYMBOLS + _lib.GRAPH_SYMBOLS + _lib.CLUSTER_SYMBOLS + _lib.DE_SYMBOLS + _lib.PCA_SYMBOLS + _lib.PCA_FIT_SYMBOLS
              + _lib.QC_SYMBOLS + _lib.LAYOUT_SYMBOLS)
    assert not set(_lib.UMAP_SYMBOLS) & set(others)
    L = _lib.lib()
    for n in _lib.UMAP_SYMBOLS:
        assert hasattr(L, n), n
    group = _umap.geometry()
    assert group in (1, 2, 4, 8, 16, 32, 64)
    assert "UM_GROUP = %d;" % group in open(os.path.join(REPO, "nabo_amd", "csrc", "umap.hip")).read()


def test_header_is_plain_c_and_links(tmp_path):
    _lib.lib()
    exe = os.path.join(str(tmp_path), "umap_check")
    cmd = ["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(REPO, "include"),
           os.path.join(REPO, "tests", "abi_c", "umap_check.c"), "-L" + os.path.join(REPO, "nabo_amd"), "-lnabo_knn",
           "-Wl,-rpath," + os.path.join(REPO, "nabo_amd"), "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0 and "%d entry points" % len(_lib.UMAP_SYMBOLS) in r.stdout, r.stdout


def graph_invariants(idx, dist, n_epochs):
    """the restated graph of one list case, after the assertions every case must pass"""
    n, k = idx.shape
    g = ur.fuzzy_graph(idx, dist, n_epochs)
    # the cases are chosen so that nothing sits on a threshold: the GPU test may then demand equality
    assert not g["flagged"].any() and not g["near"].any()
    # w is symmetric bit for bit, rows ascend, no self arc, everything within (0, 1]
    w = {(int(s), int(d)): x for s, d, x in zip(np.repeat(np.arange(n), np.diff(g["ptr"])), g["nbr"], g["w"])}
    assert len(w) == len(g["w"]) and all(w[(j, i)] == x and i != j for (i, j), x in w.items())
    for i in range(n):
        row = g["nbr"][g["ptr"][i]:g["ptr"][i + 1]]
        assert (np.diff(row) > 0).all()
    assert (g["w"] > 0).all() and g["w"].max() == g["wmax"] <= 1.0 and (g["w"] >= g["wmax"] / n_epochs).all()
    # the search met its target wherever the floor did not act; rho is the smallest positive entry
    ok = np.abs(g["psum_at"] - math.log2(k)) < 1e-5
    assert ok[~g["floored"]].all()
    for i in range(n):
        pos = dist[i][dist[i] > 0]
        assert g["rho"][i] == (pos.min() if len(pos) else 0.0)
    if n_epochs == ur.N_EPOCHS_KEEPING:
        assert len(g["w"]) == g["n_unpruned"]
    return g


@pytest.mark.parametrize("n_epochs", N_EPOCHS)
@pytest.mark.parametrize("name", list(ur.width_cases()))
def test_width_cases_keep_the_invariants_and_reach_every_width(name, n_epochs):
    """the lists that fill a width of the graph kernels or sit one above it: no row on a threshold (another seed is chosen,
    never a row excused), and between them every width, full and one over"""
    cases = ur.width_cases()
    idx, dist = cases[name]
    n, k = idx.shape
    g = graph_invariants(idx, dist, n_epochs)
    assert 200 <= n <= 300 and name == "knn_%dx%d" % (n, k) and not g["floored"].any()
    if n_epochs == ur.N_EPOCHS_PRUNING:
        assert len(g["w"]) < g["n_unpruned"], "n_epochs = %d was meant to prune" % n_epochs
    ks = sorted(c[0].shape[1] for c in cases.values())
    assert ks == [8, 9, 16, 17, 30, 32, 33] == sorted(ur.WIDTH_K)
    assert [ur.width_of(k) for k in ks] == [8, 16, 16, 32, 32, 32, 64]
    hip = open(os.path.join(REPO, "nabo_amd", "csrc", "umap.hip")).read()
    assert "return k <= 8 ? 8 : k <= 16 ? 16 : k <= 32 ? 32 : 64;" in hip      # width_of restates umap_width


@pytest.mark.parametrize("n_epochs", N_EPOCHS)
@pytest.mark.parametrize("name", list(CASES))
def test_restated_graph_keeps_its_invariants(gold, name, n_epochs):
    idx, dist = CASES[name]
    n, k = idx.shape
    g = graph_invariants(idx, dist, n_epochs)
    at = gold["graph_names"].tolist().index("%s/%d" % (name, n_epochs))
    assert int(gold["graph_n_arcs"][at]) == len(g["w"]) and int(gold["graph_flagged"][at]) == 0
    assert abs(float(gold["graph_w_sum"][at]) - g["w"].sum()) <= 1e-12 * g["w"].sum()
    if n_epochs != ur.N_EPOCHS_KEEPING and name not in ("knn_50x2", "floor_40x5"):   # (their weights all lie above wmax / 8)
        assert len(g["w"]) < g["n_unpruned"], "n_epochs = %d was meant to prune" % n_epochs
    if name == "duplicates_60x5":
        assert (dist[:, 1] == 0).any() and (g["rho"] == 0).sum() == 5 and g["floored"][g["rho"] == 0].all()
        rowsum = np.array([ur.tree_sum(r) for r in dist])
        assert g["sigma"][10] == 1e-3 * (ur.total_sum(rowsum) / (float(n) * float(k)))
    if name == "floor_40x5":
        assert g["floored"][[7, 19]].all() and (g["rho"][[7, 19]] > 0).all()
        assert g["sigma"][7] == 1e-3 * (float(ur.tree_sum(dist[7])) / 5.0)
    if name == "hub_600x4":
        assert g["ptr"][1] - g["ptr"][0] == 599 or n_epochs == ur.N_EPOCHS_PRUNING
        assert g["ptr"][1] - g["ptr"][0] > 256


def test_sums_follow_the_stated_order():
    v = np.array([0.1, 0.2, 0.3, 0.4, 0.5])
    assert ur.tree_sum(v) == ((0.1 + 0.2) + (0.3 + 0.4)) + ((0.5 + 0.0) + (0.0 + 0.0))
    r = np.arange(1, 601) * 0.1
    acc = [0.0] * 256
    for i, x in enumerate(r):
        acc[i % 256] += x
    h = 128
    while h:
        acc = [acc[c] + acc[c + h] for c in range(h)] + acc[h:]
        h //= 2
    assert ur.total_sum(r) == acc[0]


def scalar_epoch(ep, y, t, next_, nneg):
    """one epoch from the header's part D, arc by arc and sample by sample in Python floats and integers; returns the new
    positions, counts and the schedule after it"""
    n, dims, G = ep.n, len(y[0]), ep.group
    alpha = 1.0 - float(t) / float(ep.n_epochs)
    clip = lambda v: 4.0 if v > 4.0 else -4.0 if v < -4.0 else v
    out, counts = [], []
    next_, nneg = list(next_), list(nneg)
    for i in range(n):
        lanes = [[0.0] * dims for _ in range(G)]
        na = nn = ks = 0
        for e in range(int(ep.ptr[i]), int(ep.ptr[i + 1])):
            lane = lanes[(e - int(ep.ptr[i])) % G]
            if not next_[e] <= t:
                continue
            j = int(ep.nbr[e])
            D = [y[i][c] - y[j][c] for c in range(dims)]
            d2 = sum(x * x for x in D)
            c = (ep.ca * d2 ** (ep.b - 1.0)) / (ep.a * d2 ** ep.b + 1.0) if d2 > 0 else 0.0
            for x in range(dims):
                lane[x] += 2.0 * clip(c * D[x])
            na += 1
            next_[e] += float(ep.eps[e])
            m = int((t - nneg[e]) / float(ep.epn[e]))
            for p in range(m):
                kk = ur.sample(ep.seed, t, e, p, n)
                nn += 1
                ks = (ks + kk) & ur.M64
                if kk == i:
                    continue
                D = [y[i][c] - y[kk][c] for c in range(dims)]
                d2 = sum(x * x for x in D)
                c = ep.cr / ((0.001 + d2) * (ep.a * d2 ** ep.b + 1.0)) if d2 > 0 else 0.0
                for x in range(dims):
                    lane[x] += clip(c * D[x])
            nneg[e] += m * float(ep.epn[e])
        S = [float(ur.tree_sum(np.array([lanes[l][x] for l in range(G)]))) for x in range(dims)]
        out.append([y[i][x] + alpha * S[x] for x in range(dims)])
        counts.append((na, nn, ks))
    return out, counts, next_, nneg


@pytest.mark.parametrize("dims,nsr", [(2, 5), (3, 1)])
def test_restated_epoch_against_a_scalar_loop(dims, nsr):
    """the vectorised restatement takes every decision of the scalar loop (which arcs fire, how many samples, which
    nodes they name) and lands within rounding of its positions (numpy's vectorised pow may differ from Python's)"""
    idx, dist = CASES["knn_40x5"]
    g = ur.fuzzy_graph(idx, dist, 30)
    a, b = _umap.find_ab_params(1.0, 0.1)
    ep = ur.Epochs(g["ptr"], g["nbr"], g["w"], g["wmax"], 30, nsr, 1.0, a, b, 5, 4)
    y = np.random.default_rng(8).uniform(0, 10, size=(40, dims))
    y[3] = y[int(g["nbr"][g["ptr"][3]])]                    # a pair of coincident neighbours: d2 == 0
    fired = drawn = 0
    for t in range(30):
        nx, ng = ep.next.copy(), ep.nneg.copy()
        o = ep.step(y)
        want, counts, nx2, ng2 = scalar_epoch(ep, y.tolist(), t, nx.tolist(), ng.tolist())
        assert [c[0] for c in counts] == o["n_attr"].tolist() and [c[1] for c in counts] == o["n_neg"].tolist()
        assert [c[2] for c in counts] == [int(v) for v in o["idx_sum"]]
        assert nx2 == ep.next.tolist() and ng2 == ep.nneg.tolist()
        np.testing.assert_allclose(o["y"], np.array(want), rtol=0, atol=1e-12)
        fired += int(o["n_attr"].sum())
        drawn += int(o["n_neg"].sum())
        y = o["y"]
    assert fired > 100 and drawn > 100 * min(nsr, 2) and np.isfinite(y).all()


def test_schedule_follows_its_definition():
    """an arc of weight w fires about n_epochs w / wmax times, the heaviest from epoch 1 on in every epoch, and draws
    negative_sample_rate samples per firing in the long run; `advance` moves the schedule exactly as `step` does"""
    idx, dist = CASES["knn_333x15"]
    g = ur.fuzzy_graph(idx, dist, 200)
    ep = ur.Epochs(g["ptr"], g["nbr"], g["w"], g["wmax"], 200, 5, 1.0, 1.5, 0.9, 0, 16)
    fires, draws = np.zeros(ep.E, dtype=np.int64), np.zeros(ep.E, dtype=np.int64)
    for t in range(200):
        e, m = ep.firing()
        assert (m >= 0).all()
        if t == 0:
            assert len(e) == 0                               # next_e = eps_e >= 1 > 0
        fires[e] += 1
        draws[e] += m
    want = np.floor(199.0 * g["w"] / g["wmax"] + 1e-9)
    assert (np.abs(fires - want) <= 1).all() and fires[g["w"] == g["wmax"]].min() == 199
    assert (np.abs(draws - 5 * fires) <= 5).all()
    other = ur.Epochs(g["ptr"], g["nbr"], g["w"], g["wmax"], 200, 5, 1.0, 1.5, 0.9, 0, 16)
    other.advance(200)
    assert np.array_equal(other.next, ep.next) and np.array_equal(other.nneg, ep.nneg)


def test_negative_samples_follow_their_formula():
    ep = ur.Epochs([0, 1, 2, 2], [1, 0], [1.0, 1.0], 1.0, 10, 5, 1.0, 1.5, 0.9, 12345, 16)
    e = np.array([0, 1, 7, 10 ** 6], dtype=np.int64)
    for t in (0, 3, 199):
        for p in (0, 4):
            got = ep.samples(t, e, p)
            assert got.tolist() == [ur.sample(12345, t, int(x), p, 3) for x in e]
    # the same in the definition's own words, once
    mix = ur.mix_int
    z = mix(mix(mix(12345 + ur.GOLD * 4) + ur.GOLD * 8) + ur.GOLD * 5)
    assert ur.sample(12345, 3, 7, 4, 1000) == ((z >> 32) * 1000) >> 32
    draws = np.array([ur.sample(1, 0, x, 0, 10) for x in range(4000)])
    assert draws.min() == 0 and draws.max() == 9 and np.bincount(draws).min() > 300


AB = [(1.0, 0.1), (1.0, 0.5), (2.0, 0.01), (0.5, 0.3)]


@pytest.mark.parametrize("spread,min_dist", AB)
def test_curve_fit_against_scipy(gold, spread, min_dist):
    """both are least-squares minima of the same smooth problem; the generator measured the largest difference between
    the two fitted curves on the 300 points, and 10 x that covers the different stopping rules"""
    so = pytest.importorskip("scipy.optimize")
    at = [tuple(r) for r in gold["ab_cases"].tolist()].index((spread, min_dist))
    stored = float(gold["ab_curve_diff"][at])
    assert 0 <= stored < 1e-5, "tests/golden/umap.npz was written without scipy, or the fit is far off: %r" % stored
    a, b = _umap.find_ab_params(spread, min_dist)
    assert (a, b) == tuple(gold["ab_fit"][at]), "find_ab_params changed: run tools/gen_golden_umap.py"
    x, y = _umap.curve(spread, min_dist)
    f = lambda x, a, b: 1.0 / (1.0 + a * x ** (2 * b))
    p, _ = so.curve_fit(f, x, y)
    diff = float(np.max(np.abs(f(x, a, b) - f(x, *p))))
    print("spread %g, min_dist %g: a = %.9g, b = %.9g; curves differ by %.3g (stored %.3g)" % (spread, min_dist, a, b, diff, stored))
    assert diff <= 10 * stored
    # and it is a minimum: no neighbour on a small ring has a smaller sum of squares
    cost = lambda a, b: float(((f(x, a, b) - y) ** 2).sum())
    c0 = cost(a, b)
    for da, db in ((1e-4, 0), (-1e-4, 0), (0, 1e-4), (0, -1e-4)):
        assert cost(a + da, b + db) >= c0


def test_curve_and_default_epochs():
    x, y = _umap.curve(1.0, 0.1)
    assert len(x) == 300 and x[0] == 0 and x[-1] == 3.0 and (y[x < 0.1] == 1).all() and y[-1] == math.exp(-(3.0 - 0.1) / 1.0)
    assert _umap.default_n_epochs(10000) == 500 and _umap.default_n_epochs(10001) == 200


def test_start_positions():
    X = np.random.default_rng(2).normal(size=(50, 4))
    X[:, 1] = 3.5                                            # a constant column maps to 0
    y = _umap.start_positions("pca", X, 50, 3, 0)
    assert y.shape == (50, 3) and (y[:, 1] == 0).all()
    for c in (0, 2):
        assert y[:, c].min() == 0 and y[:, c].max() == 10
        assert np.array_equal(y[:, c], (10.0 * (X[:, c] - X[:, c].min())) / (X[:, c].max() - X[:, c].min()))
    r = _umap.start_positions("random", X, 50, 2, 9)
    assert np.array_equal(r, _umap.scale_start(np.random.default_rng(9).uniform(-10, 10, size=(50, 2))))
    given = _umap.start_positions(X[:, [0, 2]] * 7 + 1, None, 50, 2, 0)
    np.testing.assert_allclose(given, y[:, [0, 2]], rtol=0, atol=1e-13)


GOOD = dict(X=np.random.default_rng(1).normal(size=(30, 4)), n_neighbors=5, dims=2, n_epochs=10)


@pytest.mark.parametrize("change", [
    {"X": np.zeros(30)},                                     # not 2-D
    {"X": np.full((30, 4), np.nan)},
    {"X": np.zeros((2, 4))},                                 # too few cells
    {"n_neighbors": 1},
    {"n_neighbors": 57},                                     # above NABO_MAX_K
    {"n_neighbors": 30},                                     # not below n
    {"n_neighbors": 5.5},
    {"dims": 1},
    {"dims": 4},
    {"n_epochs": 0},
    {"negative_sample_rate": 0},
    {"repulsion_strength": np.inf},
    {"spread": 0.0},
    {"min_dist": -0.1},
    {"min_dist": 3.0},                                       # not below 3 * spread
    {"a": 1.5},                                              # a without b
    {"a": -1.0, "b": 1.0},
    {"seed": -1},
    {"init": "spectral"},
    {"init": np.zeros((30, 3))},                             # dims is 2
    {"init": np.full((30, 2), np.inf)},
    {"dims": 3, "X": np.zeros((30, 2)) + np.arange(30)[:, None]},   # the pca start needs 3 components
])
def test_bad_arguments_raise_before_any_device(change):
    with pytest.raises(ValueError) as e:
        nabo_amd.umap_fit(**dict(GOOD, **change))
    assert str(e.value).startswith("ERROR: ")


@pytest.mark.parametrize("change", [
    {"idx": np.zeros((10, 3, 1), dtype=np.int64)},
    {"dist": np.zeros((10, 4))},                             # another shape than idx
    {"idx": np.tile(np.arange(3), (10, 1)) + 10},            # no such cell
    {"idx": np.tile(np.array([0, 1, 1]), (10, 1))},          # a cell twice in a row
    {"dist": np.tile(np.array([0.0, 2.0, 1.0]), (10, 1))},   # not ascending
    {"dist": np.tile(np.array([0.0, 1.0, np.nan]), (10, 1))},
    {"dist": np.tile(np.array([-1.0, 1.0, 2.0]), (10, 1))},
    {"n_epochs": 0},
])
def test_bad_lists_raise_before_any_device(change):
    good = dict(idx=np.stack([(np.arange(3) + i) % 10 for i in range(10)]), dist=np.tile(np.array([0.0, 1.0, 2.0]), (10, 1)))
    with pytest.raises(ValueError) as e:
        nabo_amd.umap_fuzzy_graph(**dict(good, **change))
    assert str(e.value).startswith("ERROR: ")


def test_no_device_is_a_loud_failure():
    if nabo_amd.device_count() > 0:
        pytest.skip("a GPU is visible here; the no-device path is covered on the CPU box")
    with pytest.raises(nabo_amd.NaboError) as e:
        nabo_amd.umap_fit(**GOOD)
    assert "no HIP device" in str(e.value)


def test_make_umap_returns_the_reference_frame(monkeypatch):
    pd = pytest.importorskip("pandas")
    cells = ["AAAC-1", "AAAG-1", "AATT-1", "ACGT-1"]
    Z = np.arange(20.0).reshape(4, 5)
    seen = {}

    def read_cells(fn, grp, use_comps):
        seen["read"] = (fn, grp, use_comps)
        return cells, Z[:, :use_comps]

    def fit(X, n_neighbors, dims, n_epochs, spread, min_dist, repulsion_strength, negative_sample_rate, seed, init, device=0):
        seen["fit"] = dict(X=X, n_neighbors=n_neighbors, dims=dims, n_epochs=n_epochs, spread=spread, min_dist=min_dist,
                           repulsion_strength=repulsion_strength, negative_sample_rate=negative_sample_rate, seed=seed, init=init,
                           device=device)
        return np.arange(len(X) * dims, dtype=np.float64).reshape(len(X), dims)

    monkeypatch.setattr(_umap, "_read_cells", read_cells)
    monkeypatch.setattr(_umap, "umap_fit", fit)
    df = nabo_amd.make_umap("pca.h5", 3, 2, 15, 1.0, 2.0, 0.1, 200, data_group="other", index_suffix="_WT", verbose=False, seed=4)
    assert isinstance(df, pd.DataFrame) and df.shape == (4, 2)
    assert list(df.index) == [c + "_WT" for c in cells] and list(df.columns) == ["Dim1", "Dim2"]
    assert np.array_equal(df.values, np.arange(8.0).reshape(4, 2))
    assert seen["read"] == ("pca.h5", "other", 3)            # the vectors come from data_group, not from 'data'
    f = seen["fit"]
    assert f["X"].shape == (4, 3) and (f["n_neighbors"], f["dims"], f["n_epochs"], f["spread"], f["min_dist"]) == (15, 2, 200, 1.0, 0.1)
    assert (f["repulsion_strength"], f["negative_sample_rate"], f["seed"], f["init"], f["device"]) == (2.0, 5, 4, "pca", 0)
    df3 = nabo_amd.make_umap("pca.h5", 5, 3, 15, 1.0, 1.0, 0.1, None, verbose=False)
    assert list(df3.columns) == ["Dim1", "Dim2", "Dim3"] and list(df3.index) == cells and seen["read"][1] == "data"
    with pytest.raises(TypeError):
        nabo_amd.make_umap("pca.h5", 3, 2, 15, 1.0, 2.0, 0.1, 200, "data", "", False, 4)   # seed is keyword-only
