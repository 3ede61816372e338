"""The layout step (include/nabo_layout.h, nabo_amd/_layout.py) without a GPU: the tests' numpy restatement against a
scalar double loop, the first-iteration tie S == 2 T, the stop on S == 0, the margins of every GPU case, argument checks,
the no-device failure and the two file writers read back the way the reference reads them."""
import json
import math
import os
import re

import numpy as np
import pytest

import nabo_amd
from nabo_amd import _layout, _lib

import _layout_ref as lref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_public_names_and_symbols():
    for n in ("layout_fa2", "set_ref_layout", "save_layout_as_json", "save_layout_as_csv"):
        assert n in nabo_amd.__all__ and callable(getattr(nabo_amd, n))
    assert callable(nabo_amd.RefGraph.set_ref_layout)
    src = open(os.path.join(REPO, "include", "nabo_layout.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert sorted(set(re.findall(r"\b(nabo_[a-z0-9_]+)\s*\(", src))) == sorted(_lib.LAYOUT_SYMBOLS)
    L = _lib.lib()
    for n in _lib.LAYOUT_SYMBOLS:
        assert hasattr(L, n), n
    i_block, j_tile, n_splits = _layout.geometry(700)
    assert i_block % j_tile == 0 and j_tile >= 64 and 1 <= n_splits <= -(-700 // j_tile)


def scalar_step(n, pairs, x, y, dx, dy, speed, eff, oad, ewi, jtol, sr, strong, gravity):
    """include/nabo_layout.h, steps 1-7, one node and one pair at a time in Python floats; pairs: {(i, j), i <= j: w}"""
    f32 = lambda v: float(np.float32(v))
    deg = [0] * n
    for (a, b) in pairs:
        deg[a] += 1
        if a != b:
            deg[b] += 1
    mass = [1.0 + d for d in deg]
    comp = sum(mass) / n if oad else 1.0
    ndx, ndy = [0.0] * n, [0.0] * n
    for i in range(n):
        rx = ry = 0.0
        for j in range(n):
            if j == i:
                continue
            ddx, ddy = f32(x[i]) - f32(x[j]), f32(y[i]) - f32(y[j])
            d2 = max(ddx * ddx + ddy * ddy, 2.0 ** -100)
            rx += sr * mass[i] * mass[j] * ddx / d2
            ry += sr * mass[i] * mass[j] * ddy / d2
        r = math.sqrt(x[i] * x[i] + y[i] * y[i])
        f = 0.0
        if r > 0:
            f = sr * mass[i] * gravity if strong else mass[i] * gravity / r
        gx, gy = -x[i] * f, -y[i] * f
        ax = ay = 0.0
        for j in range(n):
            if j == i or (min(i, j), max(i, j)) not in pairs:
                continue
            w = pairs[(min(i, j), max(i, j))]
            e = 1.0 if ewi == 0 else w if ewi == 1 else w ** ewi
            f = -comp * e
            if oad:
                f /= mass[min(i, j)]
            ax += (x[i] - x[j]) * f
            ay += (y[i] - y[j]) * f
        ndx[i], ndy[i] = (rx + gx) + ax, (ry + gy) + ay
    swing = [mass[i] * math.sqrt((dx[i] - ndx[i]) ** 2 + (dy[i] - ndy[i]) ** 2) for i in range(n)]
    S = sum(swing)
    T = sum(0.5 * mass[i] * math.sqrt((dx[i] + ndx[i]) ** 2 + (dy[i] + ndy[i]) ** 2) for i in range(n))
    est = 0.05 * math.sqrt(n)
    jt = jtol * max(math.sqrt(est), min(10.0, est * T / (n * n)))
    if S / T > 2.0:
        if eff > 0.05:
            eff *= 0.5
        jt = max(jt, jtol)
    target = jt * eff * T / S
    if S > jt * T:
        if eff > 0.05:
            eff *= 0.7
    elif speed < 1000:
        eff *= 1.3
    speed += min(target - speed, 0.5 * speed)
    nx = [x[i] + ndx[i] * speed / (1.0 + math.sqrt(speed * swing[i])) for i in range(n)]
    ny = [y[i] + ndy[i] * speed / (1.0 + math.sqrt(speed * swing[i])) for i in range(n)]
    return nx, ny, ndx, ndy, speed, eff, S, T


@pytest.mark.parametrize("params", [
    dict(oad=True, ewi=1.0, jtol=1.0, sr=1.0, strong=False, gravity=1.0),
    dict(oad=False, ewi=0.5, jtol=0.7, sr=2.0, strong=True, gravity=0.4),
    dict(oad=True, ewi=0.0, jtol=1.0, sr=1.0, strong=False, gravity=1.0),
])
def test_restatement_against_a_scalar_double_loop(params):
    n = 7
    # arcs from both ends, the pair (1, 4) three times (0.3 is listed last), a self-loop on 2, node 6 without edges
    ptr = [0, 2, 4, 6, 7, 9, 10, 10]
    nbr = [1, 3, 4, 0, 2, 5, 0, 1, 1, 2]
    w = [0.5, 0.25, 0.9, 0.8, 0.6, 0.7, 0.35, 0.45, 0.3, 0.15]
    pairs = {(0, 1): 0.8, (0, 3): 0.35, (1, 4): 0.3, (2, 2): 0.6, (2, 5): 0.15}
    g = lref.Graph(ptr, nbr, w)
    assert g.mass.tolist() == [3, 3, 3, 2, 2, 2, 1]
    assert list(zip(g.src.tolist(), g.dst.tolist(), g.w.tolist())) == [
        (0, 1, 0.8), (0, 3, 0.35), (1, 0, 0.8), (1, 4, 0.3), (2, 5, 0.15), (3, 0, 0.35), (4, 1, 0.3), (5, 2, 0.15)]
    kw = dict(outbound_attraction_distribution=params["oad"], edge_weight_influence=params["ewi"], jitter_tolerance=params["jtol"],
              scaling_ratio=params["sr"], strong_gravity_mode=params["strong"], gravity=params["gravity"])
    s = lref.start_state(np.random.default_rng(3).random((n, 2)))
    for _ in range(5):
        o = lref.step(g, s, **kw)
        want = scalar_step(n, pairs, s["x"].tolist(), s["y"].tolist(), s["dx"].tolist(), s["dy"].tolist(), s["speed"], s["eff"], **params)
        for got, ref in zip((o["x"], o["y"], o["dx"], o["dy"], o["speed"], o["S"], o["T"]), want[:5] + want[6:]):
            np.testing.assert_allclose(got, ref, rtol=1e-13, atol=1e-13)
        assert o["eff"] == want[5]
        s = lref.state_of(o)


def test_first_iteration_sits_on_the_tie():
    """old = 0 in the first iteration, so tract_i = swing_i / 2 exactly and, summed by one tree, S == 2 T: the comparison
    S / T > 2.0 is false"""
    for n, seed in ((2, 1), (65, 2), (700, 4)):
        ptr, nbr, w, _ = lref.planted(n, seed)
        o = lref.step(lref.Graph(ptr, nbr, w), lref.start_state(np.random.default_rng(100 + seed).random((n, 2))))
        assert o["S"] == 2.0 * o["T"] and o["S"] > 0
        assert not o["S"] / o["T"] > 2.0


def test_run_stops_when_the_forces_vanish():
    """one node at the origin: no pair, no gravity, S == T == 0; the restatement stops with the position unchanged"""
    g = lref.Graph([0, 0], [], [])
    s, outs = lref.run(g, [[0.0, 0.0]], 5)
    assert len(outs) == 1 and outs[0]["stopped"] and s["x"][0] == 0 and s["y"][0] == 0 and s["speed"] == 1.0 and s["eff"] == 1.0


@pytest.fixture(scope="module")
def all_cases():
    i_block, j_tile, _ = _layout.geometry()
    return lref.cases(i_block, j_tile)


def test_cases_keep_clear_of_the_branch_thresholds(all_cases):
    """what lets the GPU test demand the restatement's `eff` after every step: from the second iteration on S/T stays
    MARGIN away from 2 and S/(jt T) from 1 (float32 pair terms move them by about 1e-5), and everything stays finite"""
    worst = [np.inf, np.inf]
    for name, c in all_cases.items():
        g = lref.Graph(c["ptr"], c["nbr"], c["w"])
        s, outs = lref.run(g, c["pos0"], lref.N_STEPS, **c["params"])
        assert len(outs) == lref.N_STEPS and np.isfinite(s["x"]).all() and np.isfinite(s["y"]).all(), name
        assert outs[0]["S"] == 2.0 * outs[0]["T"], name
        for o in outs[1:]:
            assert o["m_half"] >= lref.MARGIN and o["m_jt"] >= lref.MARGIN, (name, o["m_half"], o["m_jt"])
            worst = [min(worst[0], o["m_half"]), min(worst[1], o["m_jt"])]
        assert outs[0]["m_jt"] >= lref.MARGIN, name
    print("smallest margins: S/T from 2: %.3g, S/(jt T) from 1: %.3g" % tuple(worst))


def test_large_cases_reach_the_paths_they_were_made_for():
    """what keeps the large GPU cases from passing vacuously if the kernel's geometry changes: every split of the
    repulsion holds at least two tiles and the last split fewer than the others, and the larger case has more than 256
    node blocks, so that the speed kernel's strided loop over the block sums comes round a second time.  (Their margins
    from step 6's thresholds are asserted on the GPU, from the device's S and T: the float64 restatement of all n^2
    pairs takes minutes.)"""
    i_block, j_tile, _ = _layout.geometry()
    hip = open(os.path.join(REPO, "nabo_amd", "csrc", "layout.hip")).read()
    assert int(re.search(r"LAY_THREADS = (\d+);", hip).group(1)) == lref.NODE_BLOCK
    large = lref.large_cases(j_tile)
    assert len(large) == 2 and not set(large) & set(lref.cases(i_block, j_tile))
    most_blocks = 0
    for name, c in large.items():
        g, n = c["graph"], c["graph"].n
        n_splits = _layout.geometry(n)[2]
        ntiles, per_split, last = lref.split_geometry(n, j_tile, n_splits)
        assert ntiles == math.ceil(n / j_tile) and math.ceil(ntiles / n_splits) >= 2, name
        assert ntiles % per_split != 0 and last == ntiles % per_split and (n_splits - 1) * per_split + last == ntiles, name
        most_blocks = max(most_blocks, math.ceil(n / lref.NODE_BLOCK))
        # the graph: simple, every node on the ring, masses that differ, the arrays the device gets name the same pairs
        assert name == "ring_%d" % n and c["pos0"].shape == (n, 2) and len(c["ptr"]) == n + 1
        assert g.mass.min() >= 3 and len(np.unique(g.mass)) > 4 and len(g.src) == 2 * len(c["nbr"]) == 2 * c["ptr"][-1]
        rows = lref.sample_rows(n, i_block, j_tile, c["seed"])
        assert rows[0] == 0 and rows[-1] == n - 1 and (np.diff(rows) > 0).all() and len(rows) < 1200
        assert set(range((ntiles - 1) * j_tile, n)) <= set(rows.tolist()) and {i_block - 1, i_block, j_tile - 1, j_tile} <= set(rows.tolist())
    assert most_blocks > lref.NODE_BLOCK
    n16 = large["ring_%d" % (64 * j_tile + 1)]["graph"].n     # the smaller case: the last split is one tile of one node
    assert lref.split_geometry(n16, j_tile, _layout.geometry(n16)[2])[2] == 1 and n16 % j_tile == 1


def test_vectorised_graph_and_sampled_repulsion_equal_the_plain_ones():
    """the large cases' graph builder against Graph's Python loop, and repulsion_rows on a sample, in chunks, against the
    rows of the whole restatement"""
    ptr, nbr, w, g = lref.ring_chords(300, 5)
    plain = lref.Graph(ptr, nbr, w)
    for k in ("mass", "src", "dst", "w"):
        assert np.array_equal(getattr(g, k), getattr(plain, k)), k
    assert g.n == plain.n == 300
    s = lref.start_state(np.random.default_rng(6).random((300, 2)))
    o = lref.step(plain, s, scaling_ratio=2.5)
    rows = lref.sample_rows(300, 128, 32, 7, n_random=20)
    rep, rep_abs = lref.repulsion_rows(g, s["x"], s["y"], rows, 2.5, chunk=7)
    assert np.array_equal(rep, o["rep"][rows]) and np.array_equal(rep_abs, o["rep_abs"][rows])
    speed, eff, m_half, m_jt, _ = lref.speed_step(300, o["S"], o["T"], s["speed"], s["eff"], 1.0)
    assert (speed, eff, m_half, m_jt) == (o["speed"], o["eff"], o["m_half"], o["m_jt"])


GOOD = dict(ptr=[0, 1, 2, 2], nbr=[1, 0], w=[0.5, 0.25], pos0=[[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]], niter=2)


@pytest.mark.parametrize("change", [
    {"ptr": [0, 3, 2, 2]},                       # not monotone
    {"ptr": [1, 1, 2, 2]},                       # ptr[0] != 0
    {"ptr": [0, 1, 2, 3]},                       # ends past the arcs
    {"ptr": [[0, 1, 2, 2]]},                     # not 1-D
    {"ptr": [0]},                                # no node
    {"nbr": [1, 3]},                             # no such node
    {"nbr": [1, -1]},
    {"w": [0.5]},                                # fewer weights than arcs
    {"w": [0.5, np.nan]},
    {"w": [0.5, np.inf]},
    {"pos0": [[0.0, 0.0], [1.0, 0.0]]},          # a node without a position
    {"pos0": [0.0, 1.0, 2.0]},
    {"pos0": [[0.0, 0.0], [1.0, np.nan], [0.0, 1.0]]},
    {"niter": -1},
    {"gravity": np.inf},
    {"edge_weight_influence": "strong"},
    {"theta": 1.2},                              # no such parameter
])
def test_bad_arguments_raise_before_any_device(change):
    with pytest.raises(ValueError) as e:
        nabo_amd.layout_fa2(**dict(GOOD, **change))
    assert str(e.value).startswith("ERROR: ")


def test_no_device_is_a_loud_failure():
    if nabo_amd.device_count() > 0:
        pytest.skip("a GPU is visible here; the no-device path is covered on the CPU box")
    with pytest.raises(nabo_amd.NaboError) as e:
        nabo_amd.layout_fa2(**GOOD)
    assert "no HIP device" in str(e.value)


def test_init_pos_must_name_every_node():
    rows = ["a_r", "b_r", "c_r"]
    pos = {"a_r": 0, "b_r": 1, "c_r": 2}
    args = (rows, pos, 3, rows, np.array([0, 1, 2, 2]), np.array([1, 0]), np.array([0.5, 0.25]), 1)
    with pytest.raises(ValueError) as e:
        _layout._layout_of_graph(*args, {"a_r": (0, 0), "c_r": (1, 1)}, 0, False, 0, {})
    assert "b_r" in str(e.value)
    with pytest.raises(ValueError):
        _layout._layout_of_graph(*args, {"a_r": (0, 0), "b_r": "xy", "c_r": (1, 1)}, 0, False, 0, {})


LAYOUT = {"AAAC-1_ref": (0.0, 12.25), "AAAG-1_ref": (3.0000000000000004, 0.1), "AATT-1_ref": (1e-17, 123456.789012345)}


def test_json_writer_reads_back_as_the_reference_reads_it(tmp_path):
    fn = os.path.join(str(tmp_path), "layout.json")
    nabo_amd.save_layout_as_json(LAYOUT, fn)
    got = json.load(open(fn))                    # Graph.import_layout_from_json
    assert list(got) == list(LAYOUT)
    for k, v in got.items():                     # Graph.import_layout: a pair of floats per node
        assert len(v) == 2 and (float(v[0]), float(v[1])) == LAYOUT[k]


def test_csv_writer_reads_back_as_the_reference_reads_it(tmp_path):
    pd = pytest.importorskip("pandas")
    fn = os.path.join(str(tmp_path), "layout.csv")
    nabo_amd.save_layout_as_csv(LAYOUT, fn)
    # Graph.import_layout_from_csv with its defaults (csv_sep=',', dim_cols=(0, 1), header=None)
    layout = pd.read_csv(fn, index_col=0, sep=",", header=None)
    d1, d2 = layout.columns[0], layout.columns[1]
    got = {x: (layout[d1][x], layout[d2][x]) for x in layout.index}
    assert list(got) == list(LAYOUT)
    for k, v in got.items():
        assert (float(v[0]), float(v[1])) == LAYOUT[k]
    # and the same bytes the reference's own writer produces
    ref = os.path.join(str(tmp_path), "ref.csv")
    pd.DataFrame(LAYOUT).T.to_csv(ref, header=None)
    assert open(fn).read() == open(ref).read()
