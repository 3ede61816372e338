"""The layout on the MI355X (nabo_layout_*, nabo_amd._layout) against the tests' float64 restatement of
include/nabo_layout.h (tests/_layout_ref.py), ONE ITERATION AT A TIME: a layout is chaotic, so comparing after many
free-running iterations would test nothing.  For N_STEPS iterations the state is downloaded, the device runs one
iteration, the restatement runs one iteration from the downloaded state, and the two are compared:

  repulsion   componentwise |F_gpu - F_ref| <= (n + 16) 2^-24 sum_j |term_ij|: v_rcp_f32 and every float32 operation are
              within 1 ulp = 2^-23, at most 8 of them per term, plus at most n float32 additions of 2^-24 each.  A missed
              tile, a wrong mass or a self-term is off by orders of magnitude more;
  gravity, attraction, S, T   float64: 64 n 2^-53 of the sum of the absolute terms; only the order of summation is free.
              S and T are sums over the DEVICE's forces (old state and new dx, dy, both downloaded): the restatement's own
              S and T come from float64 pair terms and differ by the float32 error of the repulsion;
  eff         equal to the restatement's after every step: it records which branches step 6 took.  The cases keep S/T and
              S/(jt T) at least 1e-3 away from their thresholds (tests/test_layout_cpu.py asserts it on the CPU);
  x, y, speed within 4 x the largest deviation measured once on the MI355X, |x_gpu - x_ref| / max(1, the node's step
              length) over all cases (tests/golden/layout.npz, written by tools/gen_golden_layout.py), and never above 1e-3.

Two large graphs (tests/_layout_ref.large_cases; test_large_graphs_one_iteration_at_a_time states their bounds) reach what
only more than 64 tiles or more than 256 node blocks reach: several tiles in a split, a shorter last split, a second pass
over the block sums.  There the repulsion is checked on a sample of rows and everything else from the device's own forces.
"""
import numpy as np
import pytest

from nabo_amd import _layout

import _layout_ref as lref

pytestmark = pytest.mark.gpu

I_BLOCK, J_TILE, _ = _layout.geometry()
CASES = lref.cases(I_BLOCK, J_TILE)
POS_BOUND_MAX = 1e-3


def step_case(c, check=True):
    """steps one case through N_STEPS iterations on device 0; with `check` asserts every bound but the positions';
    returns the largest position / speed deviation, the figure tests/golden/layout.npz stores"""
    g = lref.Graph(c["ptr"], c["nbr"], c["w"])
    n = g.n
    f32_tol, f64_tol = (n + 16) * 2.0 ** -24, 64 * n * 2.0 ** -53
    worst = dict(rep=0.0, grav=0.0, attr=0.0, st=0.0, pos=0.0)

    def rel(err, scale):
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(err == 0, 0.0, err / scale)
        return float(np.max(r))

    with _layout.Layout(c["ptr"], c["nbr"], c["w"], **c["params"]) as L:
        L.set_state(c["pos0"][:, 0], c["pos0"][:, 1])
        for it in range(lref.N_STEPS):
            s = L.get_state()
            assert L.run(1) == 1
            f, a = L.last_forces(), L.get_state()
            o = lref.step(g, s, **c["params"])
            assert not o["stopped"]
            if it > 0:
                assert o["m_half"] >= lref.MARGIN and o["m_jt"] >= lref.MARGIN, (it, o["m_half"], o["m_jt"])
            worst["rep"] = max(worst["rep"], rel(np.abs(f["repulsion"] - o["rep"]), o["rep_abs"]) / f32_tol)
            worst["grav"] = max(worst["grav"], rel(np.abs(f["gravity"] - o["grav"]), o["grav_abs"]) / f64_tol)
            worst["attr"] = max(worst["attr"], rel(np.abs(f["attraction"] - o["attr"]), o["attr_abs"]) / f64_tol)
            # the force is the sum of its parts, and S, T are the sums over the device's own forces
            d = (f["repulsion"] + f["gravity"]) + f["attraction"]
            old = np.stack([s["dx"], s["dy"]], axis=1)
            S = float((g.mass * np.sqrt(((old - d) ** 2).sum(axis=1))).sum())
            T = float((0.5 * g.mass * np.sqrt(((old + d) ** 2).sum(axis=1))).sum())
            worst["st"] = max(worst["st"], abs(f["S"] - S) / S / f64_tol, abs(f["T"] - T) / T / f64_tol)
            steplen = np.maximum(1.0, np.hypot(o["move"][:, 0], o["move"][:, 1]))
            worst["pos"] = max(worst["pos"], float(np.max(np.abs(a["x"] - o["x"]) / steplen)), float(np.max(np.abs(a["y"] - o["y"]) / steplen)),
                               abs(a["speed"] - o["speed"]) / max(1.0, abs(o["speed"])))
            if check:
                assert np.array_equal(a["dx"], d[:, 0]) and np.array_equal(a["dy"], d[:, 1]), it
                if it == 0:
                    assert f["S"] == 2.0 * f["T"], "the first iteration must sit exactly on the tie"
                assert a["eff"] == o["eff"], (it, a["eff"], o["eff"], o["m_half"], o["m_jt"])
                assert np.isfinite(a["x"]).all() and np.isfinite(a["y"]).all()
    print("n=%d: error / bound: repulsion %.3g, gravity %.3g, attraction %.3g, S and T %.3g; position deviation %.3g"
          % (n, worst["rep"], worst["grav"], worst["attr"], worst["st"], worst["pos"]))
    if check:
        assert worst["rep"] <= 1.0 and worst["grav"] <= 1.0 and worst["attr"] <= 1.0 and worst["st"] <= 1.0, worst
    return worst["pos"]


@pytest.mark.parametrize("name", list(CASES))
def test_one_iteration_at_a_time(gpu_lib, golden, name):
    gold = golden("layout")
    assert sorted(gold["case_names"].tolist()) == sorted(CASES) and I_BLOCK == int(gold["i_block"]) and J_TILE == int(gold["j_tile"]), \
        "tests/golden/layout.npz was measured on other cases or another kernel geometry: run tools/gen_golden_layout.py"
    assert [CASES[k]["seed"] for k in gold["case_names"].tolist()] == gold["case_seeds"].tolist()
    bound = 4.0 * float(gold["pos_dev_measured"])
    assert 0.0 < bound <= POS_BOUND_MAX, "the measured deviation would need a bound above 1e-3: the kernel is wrong, not the tolerance"
    dev = step_case(CASES[name])
    assert dev <= bound, (dev, bound)


LARGE = lref.large_cases(J_TILE)
SPEED_ULPS = 10
POS_ULPS = 12


@pytest.mark.parametrize("name", list(LARGE))
def test_large_graphs_one_iteration_at_a_time(gpu_lib, name):
    """More than 64 tiles, so that a split holds several tiles and the last split fewer (the tile loop of the repulsion
    kernel comes round again, with its prefetch, its barrier and the float64 sum over tiles), and at the larger size more
    than 256 block sums (the speed kernel's strided loop comes round again); tests/test_layout_cpu.py asserts that the
    geometry makes it so.  LARGE_STEPS iterations from a seeded uniform start, one at a time.  The whole float64
    restatement is O(n^2), so:

      repulsion   a sample of rows (tests/_layout_ref.sample_rows), each against every j.  Componentwise
                  |F_gpu - F_ref| <= (j_tile + 16) 2^-24 sum_j |term_ij|: the header sums float32 within a tile only, so
                  8 roundings of 2^-23 per term and j_tile float32 additions of 2^-24 each; across tiles and splits the
                  sum is float64.  (The small cases' (n + 16) 2^-24 would be 3.9e-3 at n = 65537, the size of one tile
                  missed among 257.)
      gravity, attraction   every row, 64 n 2^-53 of the sums of the absolute terms, as for the small cases.
      dx, dy      (rep + grav) + attr of the downloaded parts, bit for bit.
      S, T        float64 sums over the device's own forces and the previous dx, dy: 64 n 2^-53.  S == 2 T in the first
                  iteration.
      eff         equal to step 6 restated from the device's S and T, which keep MARGIN from both thresholds.
      speed       within SPEED_ULPS = 10 ulp (2^-52) of max(old speed, |target|, new speed), step 6 restated from the
                  device's S and T: sqrt(n), * 0.05, then sqrt(est) or est * T / (n n), * jitter_tolerance, * eff, * T,
                  / S, - speed, + speed are at most 10 operations that round, each once on either side.
      x, y        within POS_ULPS = 12 ulp of max(|x|, |move|, |new x|), step 7 restated from the device's speed, dx, dy
                  and the swing of its dx, dy: the sum of two squares (2), sqrt, * mass, * speed, sqrt, 1 +, speed /,
                  dx *, x + are 10 operations that round once on either side (a fused multiply-add drops a rounding),
                  and 2 more for a sqrt within 1 ulp."""
    c = LARGE[name]
    g, n, p = c["graph"], c["graph"].n, dict(lref.DEFAULTS, **c["params"])
    ntiles, per_split, last = lref.split_geometry(n, J_TILE, _layout.geometry(n)[2])
    assert per_split >= 2 and 0 < last < per_split, "the case was meant to put several tiles in a split and fewer in the last"
    rows = lref.sample_rows(n, I_BLOCK, J_TILE, c["seed"])
    f32_tol, f64_tol, ulp = (J_TILE + 16) * 2.0 ** -24, 64 * n * 2.0 ** -53, 2.0 ** -52
    worst = dict(rep=0.0, grav=0.0, attr=0.0, st=0.0, speed=0.0, pos=0.0)

    def rel(err, scale):
        with np.errstate(divide="ignore", invalid="ignore"):
            return float(np.max(np.where(err == 0, 0.0, err / scale)))

    with _layout.Layout(c["ptr"], c["nbr"], c["w"], **c["params"]) as L:
        L.set_state(c["pos0"][:, 0], c["pos0"][:, 1])
        for it in range(lref.LARGE_STEPS):
            s = L.get_state()
            assert L.run(1) == 1
            f, a = L.last_forces(), L.get_state()
            rep, rep_abs = lref.repulsion_rows(g, s["x"], s["y"], rows, float(p["scaling_ratio"]), chunk=64)
            grav, attr, attr_abs = lref.local_forces(g, s["x"], s["y"], **p)
            worst["rep"] = max(worst["rep"], rel(np.abs(f["repulsion"][rows] - rep), rep_abs) / f32_tol)
            worst["grav"] = max(worst["grav"], rel(np.abs(f["gravity"] - grav), np.abs(grav)) / f64_tol)
            worst["attr"] = max(worst["attr"], rel(np.abs(f["attraction"] - attr), attr_abs) / f64_tol)
            d = (f["repulsion"] + f["gravity"]) + f["attraction"]
            assert np.array_equal(a["dx"], d[:, 0]) and np.array_equal(a["dy"], d[:, 1]), it
            old = np.stack([s["dx"], s["dy"]], axis=1)
            swing = g.mass * np.sqrt(((old - d) ** 2).sum(axis=1))
            S, T = float(swing.sum()), float((0.5 * g.mass * np.sqrt(((old + d) ** 2).sum(axis=1))).sum())
            worst["st"] = max(worst["st"], abs(f["S"] - S) / S / f64_tol, abs(f["T"] - T) / T / f64_tol)
            # step 6 from the device's S and T
            speed, eff, m_half, m_jt, target = lref.speed_step(n, f["S"], f["T"], s["speed"], s["eff"], p["jitter_tolerance"])
            if it == 0:
                assert f["S"] == 2.0 * f["T"], "the first iteration must sit exactly on the tie"
            else:
                assert m_half >= lref.MARGIN, (it, m_half)
            assert m_jt >= lref.MARGIN, (it, m_jt)
            assert a["eff"] == eff, (it, a["eff"], eff, m_half, m_jt)
            worst["speed"] = max(worst["speed"], abs(a["speed"] - speed) / (ulp * max(s["speed"], abs(target), speed)) / SPEED_ULPS)
            # step 7 from the device's speed, forces and their swing
            fac = a["speed"] / (1.0 + np.sqrt(a["speed"] * swing))
            for k, (new, was) in enumerate(((a["x"], s["x"]), (a["y"], s["y"]))):
                move = d[:, k] * fac
                scale = np.maximum(np.maximum(np.abs(was), np.abs(move)), np.abs(was + move))
                worst["pos"] = max(worst["pos"], rel(np.abs(new - (was + move)), scale) / ulp / POS_ULPS)
            assert np.isfinite(a["x"]).all() and np.isfinite(a["y"]).all()
    print("n=%d, %d tiles, %d per split, %d in the last, %d rows sampled: error / bound: repulsion %.3g, gravity %.3g, attraction %.3g, "
          "S and T %.3g, speed %.3g, positions %.3g" % (n, ntiles, per_split, last, len(rows), worst["rep"], worst["grav"], worst["attr"],
                                                        worst["st"], worst["speed"], worst["pos"]))
    assert max(worst.values()) <= 1.0, worst


def test_stops_when_the_forces_vanish(gpu_lib):
    """one node at the origin: S == T == 0 in the first iteration; nothing moves and no iteration counts"""
    with _layout.Layout([0, 0], [], []) as L:
        L.set_state([0.0], [0.0])
        assert L.run(7) == 0
        s = L.get_state()
    assert s["x"][0] == 0 and s["y"][0] == 0 and s["speed"] == 1.0 and s["eff"] == 1.0
    # two nodes drift apart for 3 iterations, then a second run goes on from the state the first left
    c = CASES["planted_2"]
    with _layout.Layout(c["ptr"], c["nbr"], c["w"]) as L:
        L.set_state(c["pos0"][:, 0], c["pos0"][:, 1])
        assert L.run(3) == 3 and L.run(2) == 2
        s = L.get_state()
    want = gpu_lib.layout_fa2(c["ptr"], c["nbr"], c["w"], c["pos0"], 5)
    assert np.array_equal(want[:, 0], s["x"]) and np.array_equal(want[:, 1], s["y"])


@pytest.fixture(scope="module")
def run_700(gpu_lib):
    c = CASES["planted_700"]
    return [gpu_lib.layout_fa2(c["ptr"], c["nbr"], c["w"], c["pos0"], 100) for _ in range(2)]


def test_two_runs_are_bit_identical(run_700):
    assert run_700[0].tobytes() == run_700[1].tobytes() and np.isfinite(run_700[0]).all()


def test_planted_groups_come_together(run_700):
    """after 100 iterations the mean distance within a planted group is below the mean distance between groups"""
    p = run_700[0]
    group = np.arange(len(p)) % 4
    d = np.hypot(p[:, None, 0] - p[None, :, 0], p[:, None, 1] - p[None, :, 1])
    same = group[:, None] == group[None, :]
    within = d[same & ~np.eye(len(p), dtype=bool)].mean()
    between = d[~same].mean()
    print("mean distance within a group %.4g, between groups %.4g" % (within, between))
    assert within < between


def test_ignored_parameters_change_nothing(gpu_lib):
    c = CASES["planted_65"]
    a = gpu_lib.layout_fa2(c["ptr"], c["nbr"], c["w"], c["pos0"], 10)
    b = gpu_lib.layout_fa2(c["ptr"], c["nbr"], c["w"], c["pos0"], 10, barnes_hut_optimize=False, barnes_hut_theta=0.3)
    assert a.tobytes() == b.tobytes()


def test_rows_in_file_order(gpu_lib):
    """what set_ref_layout does with the rows it read, without an HDF5 file: rows in an order that is not the node
    order, the seeded start dealt out in row order, the result keyed in row order and shifted to a minimum of 0"""
    c = CASES["planted_65"]
    n = len(c["ptr"]) - 1
    names = ["c%02d_WT" % i for i in range(n)]
    pos = {x: i for i, x in enumerate(names)}
    perm = np.random.default_rng(1).permutation(n)
    rows = [names[i] for i in perm]
    cut = [slice(int(c["ptr"][i]), int(c["ptr"][i + 1])) for i in perm]
    rptr = np.concatenate([[0], np.cumsum([k.stop - k.start for k in cut])]).astype(np.int64)
    rnbr, rw = np.concatenate([c["nbr"][k] for k in cut]), np.concatenate([c["w"][k] for k in cut])
    out = _layout._layout_of_graph(rows, pos, n, rows, rptr, rnbr, rw, 20, None, 4, False, 0, {})
    xy = np.array(list(out.values()))
    assert list(out) == rows and np.isfinite(xy).all() and xy[:, 0].min() == 0 and xy[:, 1].min() == 0
    raw = _layout._layout_of_graph(rows, pos, n, rows, rptr, rnbr, rw, 20, None, 4, True, 0, {})
    p0 = np.zeros((n, 2))
    p0[perm] = np.random.default_rng(4).random((n, 2))
    want = gpu_lib.layout_fa2(c["ptr"], c["nbr"], c["w"], p0, 20)
    got = np.array([raw[r] for r in rows])
    assert np.array_equal(got, want[perm]) and np.array_equal(xy, got - got.min(axis=0))
    given = _layout._layout_of_graph(rows, pos, n, rows, rptr, rnbr, rw, 20, {r: tuple(p0[pos[r]]) for r in rows}, 0, True, 0, {})
    assert given == raw


@pytest.mark.parametrize("graph_layout", ["per_node", "columnar"])
def test_set_ref_layout_on_a_mapping_file(gpu_lib, golden, tmp_path, graph_layout):
    pytest.importorskip("h5py")
    from _graph_case import build_file
    from nabo_amd._mapping import read_graph_csr
    from nabo_amd._paths import _open_ref
    import h5py
    fn, _, _ = build_file(str(tmp_path), golden("mapping_small"), graph_layout=graph_layout, tag=graph_layout)
    out = gpu_lib.set_ref_layout(fn, "WT", niter=30, verbose=False)
    with h5py.File(fn, "r") as h5:
        names, pos, uid = _open_ref(h5, "WT")
        rows, ptr, nbr, w = read_graph_csr(h5[uid + "_graph"], pos)
    assert list(out) == list(rows) and sorted(out) == sorted(names)
    xy = np.array(list(out.values()))
    assert xy.shape == (len(names), 2) and np.isfinite(xy).all() and xy[:, 0].min() == 0 and xy[:, 1].min() == 0
    with gpu_lib.RefGraph(fn, "WT") as g:
        assert g.set_ref_layout(niter=30, verbose=False) == out and g.layout == out
    # without rescaling: layout_fa2 on the same arrays (rows by node id) from the same start
    raw = gpu_lib.set_ref_layout(fn, "WT", niter=30, verbose=False, disable_rescaling=True, seed=3)
    ids = np.array([pos[r] for r in rows])
    src = np.repeat(ids, np.diff(ptr))
    order = np.argsort(src, kind="stable")
    cptr = np.concatenate([[0], np.cumsum(np.bincount(src, minlength=len(names)))])
    p0 = np.zeros((len(names), 2))
    p0[ids] = np.random.default_rng(3).random((len(names), 2))
    want = gpu_lib.layout_fa2(cptr, nbr[order], w[order], p0, 30)
    assert np.array_equal(np.array([raw[r] for r in rows]), want[ids])
    # a start that names every node is taken as given; one that misses a node is refused
    again = gpu_lib.set_ref_layout(fn, "WT", niter=30, verbose=False, disable_rescaling=True,
                                   init_pos={r: tuple(p0[pos[r]]) for r in rows})
    assert again == raw
    with pytest.raises(ValueError):
        gpu_lib.set_ref_layout(fn, "WT", niter=1, verbose=False, init_pos={r: (0.0, 0.0) for r in rows[1:]})
