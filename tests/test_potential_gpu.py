"""The differentiation potential on the MI355X (nabo_potential_*, nabo_amd._potential) against the tests' numpy
restatement of include/nabo_potential.h (tests/_potential_ref.py) and the dense route recorded in
tests/golden/potential.npz (numpy.linalg.pinv and the reference's own calc_diff_potential).

The device adds floats in another order than numpy, so nothing but integers is held to equality with the yardstick.
Every bound below is derived, with u = 2^-53 and to first order in u:
  * a row of the product, (K v)_i = c_i v_i - sum_j v_j, evaluated twice, lies within 2 (c_i + 1) u (c_i |v_i| + sum_j |v_j|)
    (pr.row_bound); a dot product a^T b evaluated twice within 2 n u sum |a_i b_i| (pr.dot_bound);
  * one iteration is held to the yardstick's FROM THE SAME STATE, the bounds above carried through alpha, beta and the
    three vector updates (iteration_bounds);
  * a whole run is held to the dense route through K e = rho: the error e of the centred iterate has
    ||e|| <= ||rho|| / lambda_2, rho = b - K x taken here from the device's x, plus 4 times the distance the golden file
    measured between the yardstick's best attainable iterate and the dense result (the dense route's own rounding; 4
    for another order of summation)."""
import warnings

import numpy as np
import pytest

from nabo_amd import _potential

import _potential_ref as pr

pytestmark = pytest.mark.gpu

GROUP, LONG, ROWS = _potential.geometry()
U = pr.U
TAGS = ("ones", "r")
NAMES = ["blob96", "blob400", "blob3000", "hub"] + ["path%d" % n for n in sorted({257, ROWS - 1, ROWS + 1})] + [
    "one_loop", "pair", "loop_beside_clique", "mapping_small"]


@pytest.fixture(scope="module")
def gold(golden):
    d = golden("potential")
    assert (int(d["long_threshold"]), int(d["block_rows"])) == (LONG, ROWS), "run tools/gen_golden_potential.py"
    assert sorted(NAMES) == sorted(str(x) for x in d["names"])
    return d


@pytest.fixture(scope="module")
def case(gold):
    """(name, tag) -> the graph, its yardstick view, r, the yardstick's b: computed once, never changed"""
    cache = {}

    def get(name, tag):
        if (name, tag) not in cache:
            if name not in cache:
                ptr, nbr = gold[name + "_ptr"].astype(np.int64), gold[name + "_nbr"].astype(np.int64)
                cache[name] = (ptr, nbr, pr.Graph(ptr, nbr))
            ptr, nbr, G = cache[name]
            r = None if tag == "ones" else gold[name + "_r"]
            cache[(name, tag)] = (ptr, nbr, G, r, pr.rhs(G, r))
        return cache[(name, tag)]
    return get


def b_bound(G, r):
    """|b_dev - b_yardstick| per node.  b_i = d_i (r_i - d_i (S1 / S2)), S1 = sum_C d r a float sum of m = |C| terms, good
    to m u sum_C |d r|; S2 exact.  The ratio is good to E = (m + 3) u sum_C |d r| / S2; r'_i to d_i E + 2 u (|r_i| + d_i
    sum_C |d r| / S2); b_i to d_i times that plus u |b_i|: per evaluation d_i (d_i E + 3 u (|r_i| + d_i sum_C |d r| / S2)),
    twice that for two."""
    r = np.ones(G.n) if r is None else np.asarray(r, dtype=np.float64)
    d = G.d.astype(np.float64)
    s1abs, s2 = G.comp_sum(np.abs(d * r)), G.comp_sum(d * d)
    ratio_abs = (s1abs / s2)[G.comp]
    E = ((G.size + 3) * U)[G.comp] * ratio_abs
    return 2.0 * d * (d * E + 3.0 * U * (np.abs(r) + d * ratio_abs))


def iteration_bounds(G, st, y):
    """how far the device's state after one iteration from `st` may lie from the yardstick's `y` (a PCG that took the
    same step); every term is first order in u, the cross terms of two errors are added where two errors multiply"""
    L = y.last
    p, q, alpha, beta, z = L["p_old"], L["q"], L["alpha"], L["beta"], L["z"]
    Eq = pr.row_bound(G, p)
    Epq = pr.dot_bound(p, q) + float((np.abs(p) * Eq).sum())
    assert Epq < 1e-6 * L["pq"]                                          # first order is enough
    Ea = abs(alpha) * (Epq / L["pq"]) * (1 + 1e-6) + 2 * U * abs(alpha)
    Ex = np.abs(p) * Ea + 4 * U * (np.abs(alpha * p) + np.abs(y.x))
    Eres = np.abs(q) * Ea + abs(alpha) * Eq + Ea * Eq + 4 * U * (np.abs(alpha * q) + np.abs(y.res))
    Ez = Eres * G.invc + 2 * U * np.abs(z)
    Erho = pr.dot_bound(y.res, z) + float((np.abs(z) * Eres + np.abs(y.res) * Ez + Eres * Ez).sum())
    Eb = Erho / L["rho_old"] + 2 * U * abs(beta)
    Ep = Ez + np.abs(p) * Eb + 4 * U * (np.abs(beta * p) + np.abs(y.p))
    return {"x": Ex, "res": Eres, "p": Ep, "rho": Erho}


def run_bound(G, b, x, lam2, delta):
    """||rho|| / lambda_2 + 4 delta, rho = b - K x"""
    rho = float(np.linalg.norm(b - G.product(x)))
    return (rho / lam2 if np.isfinite(lam2) else 0.0) + 4.0 * delta


@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("name", NAMES)
def test_prepare(gpu_lib, case, name, tag):
    ptr, nbr, G, r, b = case(name, tag)
    with _potential.Potential(ptr, nbr) as H:
        assert H.graph_size()[:2] == (G.n, len(G.src))
        H.prepare(r)
        d = H.get_prepared()
        info = H.info()
        st = H.get_state()
    assert np.array_equal(d["label"], G.label) and np.array_equal(d["d"], G.d) and np.array_equal(d["c"], G.c)
    assert info["n_components"] == len(G.roots) and info["iterations"] == 0
    bound = b_bound(G, r)
    worst = np.abs(d["b"] - b) - bound
    print("%s %s: max |b_dev - b| = %.3g, least slack %.3g" % (name, tag, np.abs(d["b"] - b).max(), -worst.max()))
    assert (worst <= 0).all()
    # the start of the iteration: x = 0, res = b, p = M^-1 b, rho = res^T p
    assert not st["x"].any() and np.array_equal(st["res"], d["b"]) and st["it"] == 0
    if np.linalg.norm(b) > 0:
        assert info["status"] == "running"
        assert (np.abs(st["p"] - d["b"] * G.invc) <= U * np.abs(st["p"])).all()
        assert abs(st["rho"] - np.dot(st["res"], st["p"])) <= pr.dot_bound(st["res"], st["p"])
    else:
        assert info["status"] == "converged"


def test_hub_graph_takes_the_workgroup_path(gpu_lib, case):
    ptr, nbr, G, _, _ = case("hub", "r")
    m = LONG + 300
    # a ring node has its two ring neighbours, the hub, and at most the two rows at the threshold
    assert G.c[m] == m and G.c[m + 1] == LONG and G.c[m + 2] == LONG + 1 and G.c[:m].max() <= 5
    with _potential.Potential(ptr, nbr) as H:
        assert H.graph_size() == (m + 3, len(G.src), 2)
    ptr, nbr, G, _, _ = case("blob400", "r")
    with _potential.Potential(ptr, nbr) as H:
        assert H.graph_size()[2] == 0 and G.c.max() <= LONG


@pytest.mark.parametrize("name,tag", [("blob96", "ones"), ("blob400", "r"), ("hub", "r"), ("path%d" % (ROWS + 1), "r"),
                                      ("path%d" % (ROWS - 1), "ones"), ("loop_beside_clique", "r"), ("mapping_small", "r")])
def test_one_iteration_at_a_time(gpu_lib, case, name, tag):
    """the first three iterations and two late ones, each from the yardstick's state"""
    ptr, nbr, G, r, b = case(name, tag)
    trace = []
    pr.PCG(G, b, 1e-10, 10000).run(trace=trace)
    picks = sorted(set(k for k in (0, 1, 2, len(trace) // 2, len(trace) - 1) if 0 <= k < len(trace)))
    assert len(picks) >= min(4, len(trace))
    with _potential.Potential(ptr, nbr, tol=1e-10) as H:
        H.prepare(r)
        for k in picks:
            st = trace[k]
            H.set_state(st["x"], st["res"], st["p"], st["rho"], st["it"])
            H.iterate(1)
            got = H.get_state()
            y = pr.PCG(G, b, 1e-10, 10000)
            y.x, y.res, y.p, y.rho, y.it = st["x"].copy(), st["res"].copy(), st["p"].copy(), st["rho"], st["it"]
            y.step()
            E = iteration_bounds(G, st, y)
            assert got["it"] == y.it == st["it"] + 1
            for v in ("x", "res", "p"):
                worst = np.abs(got[v] - getattr(y, v)) - E[v]
                at = int(np.argmax(worst))
                assert worst[at] <= 0, "iteration %d: %s[%d] is %.17g, the yardstick has %.17g, bound %.3g" % (
                    k + 1, v, at, got[v][at], getattr(y, v)[at], E[v][at])
            assert abs(got["rho"] - y.rho) <= E["rho"], "iteration %d: rho %.17g, the yardstick has %.17g, bound %.3g" % (
                k + 1, got["rho"], y.rho, E["rho"])


def test_more_partial_sums_than_one_pass_of_the_scalar_kernel(gpu_lib):
    """more than 256 workgroups: the one-workgroup kernel walks the partial sums in strides.  7 300 kites (a clique of 8
    and a pendant node) converge in a handful of iterations however many there are; every iteration is held to the
    yardstick's from the same state, and the run to its count"""
    count = (256 * ROWS) // 9 + 20
    ptr, nbr = pr.kites_graph(count)
    G = pr.Graph(ptr, nbr)
    assert (G.n + ROWS - 1) // ROWS > 256 and len(G.roots) == count and G.c.max() == 8
    r = np.random.default_rng(12).normal(size=G.n) * 2.0 + 0.25
    b = pr.rhs(G, r)
    trace = []
    ref = pr.PCG(G, b, 1e-10, 10000).run(trace=trace)
    assert ref.status == pr.CONVERGED and 2 <= ref.it <= 12
    with _potential.Potential(ptr, nbr) as H:
        H.prepare(r)
        d = H.get_prepared()
        assert np.array_equal(d["label"], G.label) and (np.abs(d["b"] - b) <= b_bound(G, r)).all()
        bb = b_bound(G, r)
        assert abs(H.get_state()["rho"] - trace[0]["rho"]) <= pr.dot_bound(b, b * G.invc) + float((2 * np.abs(b) * G.invc * bb + bb * bb).sum())
        for st in trace:
            H.set_state(st["x"], st["res"], st["p"], st["rho"], st["it"])
            H.iterate(1)
            got = H.get_state()
            y = pr.PCG(G, b, 1e-10, 10000)
            y.x, y.res, y.p, y.rho, y.it = st["x"].copy(), st["res"].copy(), st["p"].copy(), st["rho"], st["it"]
            y.step()
            E = iteration_bounds(G, st, y)
            assert got["it"] == y.it
            assert all((np.abs(got[v] - getattr(y, v)) <= E[v]).all() for v in ("x", "res", "p")) and abs(got["rho"] - y.rho) <= E["rho"]
        V, info = H.solve(r)
        x = H.get_state()["x"]
    assert info["status"] == "converged" and abs(info["iterations"] - ref.it) <= 2 and info["n_components"] == count
    # every component has the same 9 x 9 matrix: the dense pinv of one, taken here, serves them all; its own rounding is
    # taken as 16 n u times the condition of K (lambda_max <= 2 max c = 16, over lambda_2) on ||V||, n = 9
    one = pr.Graph(*pr.kites_graph(1))
    P, lam2 = np.linalg.pinv(one.dense_L()), pr.lambda2(one)
    ref_V = (r.reshape(count, 9) @ P.T).ravel()
    delta = 16 * 9 * U * (16.0 / lam2) * float(np.linalg.norm(ref_V))
    assert np.linalg.norm(V - ref_V) <= run_bound(G, b, x, lam2, delta)


@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("name", NAMES)
def test_whole_run(gpu_lib, gold, case, name, tag):
    ptr, nbr, G, r, b = case(name, tag)
    key = "%s_%s_" % (name, tag)
    with _potential.Potential(ptr, nbr, tol=1e-10) as H:
        V, info = H.solve(r)
        x = H.get_state()["x"]
    assert info["status"] == "converged" and np.isfinite(V).all()
    ref_it = int(gold[key + "iterations"])
    print("%s %s: %d iterations (yardstick %d), residual %.3g, true residual %.3g" % (name, tag, info["iterations"], ref_it,
                                                                                      info["residual"], info["true_residual"]))
    assert abs(info["iterations"] - ref_it) <= 2
    bnorm = float(np.linalg.norm(b))
    if bnorm == 0.0:
        assert info["iterations"] == 0 and not V.any() and info["true_residual"] == 0.0
    else:
        assert info["residual"] <= 1e-10
        # the reported true residual against the one recomputed here from x: the vector b - K x per entry within the
        # row bound, the bound of b and one rounding; its norm, and ||b||, each good to (n + 2) u relative
        t = b - G.product(x)
        Et = pr.row_bound(G, x) + b_bound(G, r) + 2 * U * np.abs(t)
        mine = float(np.linalg.norm(t)) / bnorm
        assert abs(info["true_residual"] - mine) <= float(np.linalg.norm(Et)) / bnorm + 4 * (G.n + 2) * U * mine
    lam2 = float(gold[name + "_lambda2"])
    for what in ("pinv", "ref"):
        err, bound = float(np.linalg.norm(V - gold[key + what])), run_bound(G, b, x, lam2, float(gold[key + "delta_" + what]))
        print("    ||V - %s|| = %.3g, bound %.3g" % (what, err, bound))
        assert err <= bound
    assert info["ms"]["run"] > 0 or bnorm == 0.0


def test_max_iter_stops_the_run_and_warns(gpu_lib, case):
    ptr, nbr, G, r, b = case("path257", "r")
    with pytest.warns(RuntimeWarning) as rec:
        V, info = gpu_lib.diff_potential_csr(ptr, nbr, r, max_iter=10)
    assert info["status"] == "max_iter" and info["iterations"] == 10 and "max_iter" in str(rec[0].message)
    assert ("%.3g" % info["true_residual"]) in str(rec[0].message) and info["true_residual"] > 1e-3
    # the iterate returned is the tenth, not a later one: ten iterations by hand, then more that change nothing
    with _potential.Potential(ptr, nbr, max_iter=10) as H:
        H.prepare(r)
        for k in range(10):
            assert H.iterate(1) == (k == 9)
        st = H.get_state()
        assert H.iterate(5) and H.get_state()["x"].tobytes() == st["x"].tobytes() and H.info()["iterations"] == 10
        assert H.finish().tobytes() == V.tobytes()
    # a converged run issues no warning
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        gpu_lib.diff_potential_csr(ptr, nbr, r)


@pytest.mark.parametrize("name", ["blob400", "hub", "path257"])
def test_two_runs_are_bit_identical_and_equal_stepping_by_hand(gpu_lib, case, name):
    ptr, nbr, G, r, b = case(name, "r")
    with _potential.Potential(ptr, nbr) as H:
        a, ia = H.solve(r)
        xa = H.get_state()
        c, ic = H.solve(r)
        assert a.tobytes() == c.tobytes() and ia["iterations"] == ic["iterations"] and ia["true_residual"] == ic["true_residual"]
        for chunk in (1, 7):                                  # the host looks at the state between any two iterations
            H.prepare(r)
            while not H.iterate(chunk):
                H.get_state()
            st = H.get_state()
            assert st["it"] == ia["iterations"] and all(st[v].tobytes() == xa[v].tobytes() for v in ("x", "res", "p"))
            assert H.finish().tobytes() == a.tobytes() and H.info()["true_residual"] == ia["true_residual"]
    V, info = gpu_lib.diff_potential_csr(ptr, nbr, r)
    assert V.tobytes() == a.tobytes() and info["iterations"] == ia["iterations"]


def test_input_forms_give_the_same_bits(gpu_lib, case):
    ptr, nbr, G, r, b = case("blob96", "r")
    base, info = gpu_lib.diff_potential_csr(ptr, nbr, r)
    n = G.n
    row = np.repeat(np.arange(n), np.diff(ptr))
    pairs = sorted(set((min(i, j), max(i, j)) for i, j in zip(row.tolist(), nbr.tolist())))
    one_way = pr.csr_of_edges(n, pairs)
    both = pr.csr_of_edges(n, pairs + [(j, i) for i, j in pairs if i != j])
    twice = pr.csr_of_edges(n, [(j, i) for i, j in pairs] + pairs[::-1] + pairs[:50])
    for g in (one_way, both, twice):
        V, i2 = gpu_lib.diff_potential_csr(g[0], g[1], r)
        assert V.tobytes() == base.tobytes() and i2["iterations"] == info["iterations"]
    # r = None is r = all ones
    a, _ = gpu_lib.diff_potential_csr(ptr, nbr, None)
    c, _ = gpu_lib.diff_potential_csr(ptr, nbr, np.ones(n))
    assert a.tobytes() == c.tobytes() and a.any()
    # a negative r gives the mirrored potential exactly: every step is odd in r, and rounding to nearest is symmetric
    neg, _ = gpu_lib.diff_potential_csr(ptr, nbr, -np.abs(r))
    pos, _ = gpu_lib.diff_potential_csr(ptr, nbr, np.abs(r))
    assert np.array_equal(neg, -pos) and (neg != 0).any()
    # r proportional to d: b = 0, no iteration, V = 0
    V, i0 = gpu_lib.diff_potential_csr(ptr, nbr, 2.5 * G.d)
    assert i0["iterations"] == 0 and i0["status"] == "converged" and not V.any() and i0["true_residual"] == 0.0


def test_small_and_degenerate_graphs(gpu_lib):
    V, info = gpu_lib.diff_potential_csr([0, 1], [0], [3.0])                          # one node and its loop
    assert V.tolist() == [0.0] and info["iterations"] == 0 and info["n_components"] == 1
    # two nodes: L = [[1, -1], [-1, 1]], pinv(L) = L / 4, V = (r0 - r1) / 4 (1, -1)
    V, info = gpu_lib.diff_potential_csr([0, 1, 1], [1], [3.0, -1.0])
    assert np.abs(V - np.array([1.0, -1.0])).max() <= 8 * U and info["iterations"] == 1 and info["status"] == "converged"
    # a lone looped node beside a triangle with r = (5, 1, 2, 3): the loner gets 0; in the triangle L = I - A/2,
    # pinv(L) = (2/3) (I - J/3), V = (2/3) (r - mean r)
    V, info = gpu_lib.diff_potential_csr(*pr.csr_of_edges(4, [(0, 0), (1, 2), (2, 3), (3, 1)]), r=[5.0, 1.0, 2.0, 3.0])
    assert info["n_components"] == 2 and V[0] == 0.0 and np.abs(V[1:] - np.array([-2.0, 0.0, 2.0]) / 3.0).max() <= 16 * U
    with pytest.raises(ValueError) as e:                                                 # node 2 has no edge
        gpu_lib.diff_potential_csr([0, 1, 2, 2], [1, 0])
    assert "node 2 has no edge" in str(e.value)


def test_dict_by_node_name_on_the_mapping_graph(gpu_lib, gold, case):
    """what calc_diff_potential does with the graph it read, without an HDF5 file: the dict is keyed in the rows' order
    and holds the reference's values"""
    ptr, nbr, G, r, b = case("mapping_small", "r")
    nodes = [str(x) for x in gold["mapping_small_nodes"]]
    pos = {x: i for i, x in enumerate(nodes)}
    rows = [nodes[i] for i in np.random.default_rng(4).permutation(G.n)]
    lam2 = float(gold["mapping_small_lambda2"])
    for tag, rd in (("ones", None), ("r", {x: float(r[pos[x]]) for x in nodes})):
        V = _potential._potential_of_graph(rows, pos, ptr, nbr, rd, 1e-10, 10000, 0)
        assert list(V) == rows
        vec = np.array([V[x] for x in nodes])
        direct, _ = gpu_lib.diff_potential_csr(ptr, nbr, None if rd is None else r)
        assert vec.tobytes() == direct.tobytes()
        ref = gold["mapping_small_%s_ref" % tag]
        # x is not kept by the one-call form; V differs from it by a constant, which K does not see
        assert np.linalg.norm(vec - ref) <= run_bound(G, case("mapping_small", tag)[4], vec, lam2, float(gold["mapping_small_%s_delta_ref" % tag]))


@pytest.mark.parametrize("graph_layout", ["per_node", "columnar"])
def test_calc_diff_potential_on_a_mapping_file(gpu_lib, golden, gold, tmp_path, graph_layout):
    pytest.importorskip("h5py")
    from _graph_case import build_file
    from nabo_amd import _community
    fn, _, _ = build_file(str(tmp_path), golden("mapping_small"), graph_layout=graph_layout, tag=graph_layout)
    ref_nodes, pos, n_ref, ptr, nbr, _ = _community._ref_graph_csr(fn, "WT")
    G = pr.Graph(ptr, nbr)
    lam2 = pr.lambda2(G)
    names = [str(x) for x in gold["mapping_small_nodes"]]
    assert sorted(names) == sorted(ref_nodes)
    rd = {x: float(v) for x, v in zip(names, gold["mapping_small_r"])}
    for tag, r in (("ones", None), ("r", rd)):
        V = gpu_lib.calc_diff_potential(fn, "WT", r)
        assert list(V) == ref_nodes                                       # the reference's node order: refNodes, the file's
        vec = np.array([V[x] for x in ref_nodes])
        ref = dict(zip(names, gold["mapping_small_%s_ref" % tag].tolist()))
        rvec = None if r is None else np.array([r[x] for x in sorted(pos, key=pos.get)])
        bound = run_bound(G, pr.rhs(G, rvec), np.array([V[x] for x in sorted(pos, key=pos.get)]), lam2,
                          float(gold["mapping_small_%s_delta_ref" % tag]))
        assert np.linalg.norm(vec - np.array([ref[x] for x in ref_nodes])) <= bound
        with gpu_lib.RefGraph(fn, "WT") as g:
            assert g.calc_diff_potential(r) == V
    assert gpu_lib.calc_diff_potential(fn, "WT", {x: 1.0 for x in ref_nodes[1:]}) == {}
