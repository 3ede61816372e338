"""Edge bundling on the device (nabo_amd/csrc/bundle.hip) against the yardstick (tests/_bundle_ref.py), one step at a
time: every step starts from the yardstick's state through set_points.  Integers (offsets, every m, counts) must be equal
and floats bit-equal: every operation of the definition is one correctly rounded IEEE operation on gfx950, and
tests/test_bundle_cpu.py has checked on the yardstick that no integer decision of these inputs sits on a threshold."""
import hashlib

import numpy as np
import pytest

from nabo_amd import _bundle

import _bundle_case as bc
import _bundle_ref as br

pytestmark = pytest.mark.gpu


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def handle(off, pts, **params):
    B = _bundle.Bundle(*bc.dummy_graph(len(off) - 1), **params)
    B.set_points(off, pts)
    return B


def check_state(B, off, pts):
    goff, gpts = B.get_points()
    assert np.array_equal(goff, off), "offsets differ: first at edge %d" % int(np.flatnonzero(goff != off)[0] if goff.shape == off.shape else -1)
    assert same_bits(gpts, pts), "points differ by at most %g" % np.abs(gpts - pts).max()


@pytest.mark.parametrize("E", bc.RESAMPLE_E)
def test_resample(gpu_lib, E):
    off, pts = bc.polylines(E)
    want = br.resample(off, pts, bc.TL)
    cap = _bundle.geometry()["short_cap"]
    if E >= 15:   # both kernels and the hand-over between them are in play
        m0, m1 = np.diff(off), np.diff(want[0])
        assert (m1 <= cap)[m0 <= cap].any() and (m1 > cap)[m0 <= cap].any() and (m0 > cap).any()
    with handle(off, pts) as B:
        again = B.get_points()
        assert np.array_equal(again[0], off) and same_bits(again[1], pts)
        B.resample()
        check_state(B, *want)
        B.resample()   # from the device's own state
        check_state(B, *br.resample(*want, bc.TL))


def test_resample_special_polylines(gpu_lib):
    off, pts = bc.special_polylines()
    want = br.resample(off, pts, bc.TL)
    assert list(np.diff(want[0])) == [2, 2, 3, br.P_MAX, 15, 2]
    with handle(off, pts) as B:
        B.resample()
        check_state(B, *want)


@pytest.mark.parametrize("chunk", [1, 7, 64])
def test_chunks_change_nothing(gpu_lib, chunk):
    off, pts = bc.polylines(65)
    with handle(off, pts) as B:
        B.set_option("chunk_edges", chunk)
        B.resample()
        check_state(B, *br.resample(off, pts, bc.TL))
        with pytest.raises(ValueError):
            B.set_option("chunk_edges", 0)
        with pytest.raises(ValueError):
            B.set_option("no_such", 1)


def test_set_points_is_checked(gpu_lib):
    off, pts = bc.polylines(3)
    with handle(off, pts) as B:
        bad = pts.copy()
        bad[1, 0] = 1.0000001
        with pytest.raises(ValueError):
            B.set_points(off, bad)
        bad[1, 0] = np.nan
        with pytest.raises(ValueError):
            B.set_points(off, bad)
        with pytest.raises(ValueError):
            B.set_points(np.array([0, 1, 3, 5]), pts[:5])
        with pytest.raises(ValueError):
            B.set_points(np.array([0, 2, 4, 517]), np.full((517, 2), 0.5))
        with pytest.raises(ValueError):
            B.advect(1)   # no field yet
        with pytest.raises(ValueError):
            B.field(3.0)  # no density yet
        check_state(B, off, pts)


@pytest.mark.parametrize("A", [7, 64, 500])
@pytest.mark.parametrize("kind", ["one_pixel", "ones", "random"])
def test_density(gpu_lib, A, kind):
    off, pts = bc.density_points(kind, A)
    want = br.density(pts, A)
    if kind == "one_pixel":
        assert want.max() == 4096 and (want > 0).sum() == 1
    if kind == "ones":
        assert want[A, :].sum() > 0 and want[:, A].sum() > 0 and want[0, 0] > 0
    with handle(off, pts, accuracy=A) as B:
        got = B.density()
        assert got.dtype == np.uint32 and np.array_equal(got, want) and int(got.sum()) == len(pts)


@pytest.mark.parametrize("A,b", [(7, 24.0), (64, 4.0), (500, 35.0)])
def test_field(gpu_lib, A, b):
    off, pts = bc.polylines(64)
    img = br.density(pts, A)
    wB, wGX, wGY = br.field(img, b)
    if A == 7:
        assert len(br.blur_weights(b)) // 2 > A
    with handle(off, pts, accuracy=A) as B:
        assert np.array_equal(B.density(), img)
        gB, gGX, gGY = B.field(b)
    assert same_bits(gB, wB), np.abs(gB - wB).max()
    assert same_bits(gGX, wGX) and same_bits(gGY, wGY), (np.abs(gGX - wGX).max(), np.abs(gGY - wGY).max())


@pytest.mark.parametrize("n_steps,every", [(1, 2), (2, 1), (2, 2)])
def test_advect(gpu_lib, n_steps, every):
    A, b = 64, 4.0
    off, pts = bc.advect_state(A)
    _, GX, GY = br.field(br.density(pts, A), b)
    one = br.advect_step(off, pts, GX, GY, A)[br.interior(off, len(pts))]
    assert (one == 0.0).any() and (one == 1.0).any()   # the step clamps at both ends
    want = br.advect(off, pts, GX, GY, A, n_steps, every, bc.TL)
    with handle(off, pts, accuracy=A, resample_every=every) as B:
        B.density()
        B.field(b)
        B.advect(n_steps)
        check_state(B, *want)


@pytest.mark.parametrize("passes", [1, 10])
def test_smooth(gpu_lib, passes):
    off, pts = bc.smooth_state()
    assert list(np.diff(off)[:2]) == [2, 3]
    with handle(off, pts) as B:
        B.smooth(passes)
        check_state(B, off, br.smooth(off, pts, 0.3, passes))
        B.smooth(0)
        check_state(B, off, br.smooth(off, pts, 0.3, passes))


@pytest.fixture(scope="module")
def runs(gpu_lib):
    pos, src, dst = bc.graph()
    return {A: gpu_lib.hammer_bundle(pos, src, dst, accuracy=A) for A in bc.RUN_A}


@pytest.mark.parametrize("A", bc.RUN_A)
def test_whole_run(gpu_lib, golden, runs, A):
    """every operation proved exact, so the yardstick's whole run (tools/gen_golden_bundle.py) is held to the byte"""
    g = golden("bundle")
    pos, src, dst = bc.graph()
    pts, off = runs[A]
    assert off.dtype == np.int64 and pts.dtype == np.float64 and pts.shape == (off[-1] + len(src), 2)
    assert np.isnan(pts[off[1:] + np.arange(len(src))]).all() and np.isfinite(pts).sum() == 2 * off[-1]
    fig = br.figures(pts, off, bc.LONG, pos, src, dst)
    print("A = %d: figures %s, the yardstick's %s, margin %s" % (A, fig, g["figures_%d" % A], g["figure_margin_%d" % A]))
    assert np.array_equal(off, g["offsets_%d" % A])
    assert hashlib.sha256(pts.tobytes()).hexdigest() == str(g["sha256_%d" % A])
    # the end points are the nodes' own positions up to the normalisation's round trip
    first = pts[off[:-1] + np.arange(len(src))]
    assert np.abs(first - pos[src]).max() < 1e-13 * np.abs(pos).max()


def test_the_same_call_twice_gives_the_same_bytes(gpu_lib, runs):
    pos, src, dst = bc.graph()
    pts, off = gpu_lib.hammer_bundle(pos, src, dst, accuracy=64)
    assert np.array_equal(off, runs[64][1]) and same_bits(pts, runs[64][0])


@pytest.mark.parametrize("A", bc.RUN_A)
def test_permuted_edges_give_permuted_polylines(gpu_lib, runs, A):
    pos, src, dst = bc.graph()
    perm = np.random.default_rng(3).permutation(len(src))
    pts, off = gpu_lib.hammer_bundle(pos, src[perm], dst[perm], accuracy=A)
    wpts, woff = runs[A]
    assert np.array_equal(np.diff(off), np.diff(woff)[perm])
    for k in (0, 1, 500, 2299):
        e = perm[k]
        assert same_bits(pts[off[k] + k:off[k + 1] + k], wpts[woff[e] + e:woff[e + 1] + e])
    pieces = [wpts[woff[e] + e:woff[e + 1] + e + 1] for e in perm]
    assert same_bits(pts, np.concatenate(pieces))


def test_steps_compose_to_the_run(gpu_lib, runs):
    """the handle stepped by hand through the definition's run gives what `run` gives, and the phases are timed"""
    pos, src, dst = bc.graph()
    with _bundle.Bundle(pos, src, dst, accuracy=64) as B:
        B.resample()
        d = 0.7
        for _ in range(4):
            b = (0.05 * d) * 64.0
            d = d * 0.7
            if b < 2:
                break
            B.density()
            B.field(b)
            B.advect(50)
        B.smooth(10)
        pts, off = B.result()
        assert np.array_equal(off, runs[64][1]) and same_bits(pts, runs[64][0])
    with _bundle.Bundle(pos, src, dst, accuracy=64) as B:
        B.run()
        ms = B.last_ms()
        assert all(ms[k] > 0 for k in _bundle.PHASES) and abs(ms["total"] - sum(ms[k] for k in _bundle.PHASES)) < 1e-6 * ms["total"]
        img = B.density()
        assert int(img.sum()) == runs[64][1][-1]


@pytest.mark.parametrize("graph_layout", ["per_node", "columnar"])
def test_bundle_edges_on_a_mapping_file(gpu_lib, golden, tmp_path, graph_layout):
    pytest.importorskip("h5py")
    from _graph_case import build_file
    from nabo_amd._mapping import read_graph_csr
    from nabo_amd._paths import _open_ref
    import h5py
    fn, _, _ = build_file(str(tmp_path), golden("mapping_small"), graph_layout=graph_layout, tag=graph_layout)
    with h5py.File(fn, "r") as h5:
        names, pos, uid = _open_ref(h5, "WT")
        rows, ptr, nbr, w = read_graph_csr(h5[uid + "_graph"], pos)
    rng = np.random.default_rng(11)
    layout = {r: (float(x), float(y)) for r, (x, y) in zip(rows, rng.random((len(rows), 2)) * 50)}
    layout[rows[3]] = None                       # a node without a position: its edges are not drawn
    cut = float(np.median(w))
    # the rule, restated: each undirected pair once where the file lists it first, the weight it lists last
    a = np.repeat([pos[r] for r in rows], np.diff(ptr))
    seen, order = {}, []
    for k, (i, j) in enumerate(zip(a, nbr)):
        key = (min(i, j), max(i, j))
        if key not in seen:
            order.append(key)
            seen[key] = [i, j, None]
        seen[key][2] = w[k]
    have = [i for i, n in enumerate(names) if layout.get(n) is not None]
    local = {i: k for k, i in enumerate(have)}
    edges = [(local[i], local[j]) for i, j, wt in (seen[k] for k in order) if wt > cut and i in local and j in local]
    assert len(edges) > 10 and len(have) == len(names) - 1
    xy = np.array([layout[names[i]] for i in have])
    want = gpu_lib.hammer_bundle(xy, [e[0] for e in edges], [e[1] for e in edges], initial_bandwidth=0.1, decay=0.7, accuracy=100)
    got = gpu_lib.bundle_edges(fn, "WT", layout, edge_min_weight=cut, accuracy=100)
    assert np.array_equal(got[1], want[1]) and same_bits(got[0], want[0])
    json_fn = str(tmp_path / "layout.json")
    gpu_lib.save_layout_as_json(layout, json_fn)
    again = gpu_lib.bundle_edges(fn, "WT", json_fn, edge_min_weight=cut, accuracy=100)
    assert same_bits(again[0], want[0])
    with gpu_lib.RefGraph(fn, "WT") as g:
        with pytest.raises(ValueError):
            g.bundle_edges()
        g.layout = layout
        mine = g.bundle_edges(edge_min_weight=cut, accuracy=100)
        assert np.array_equal(mine[1], want[1]) and same_bits(mine[0], want[0])
    with pytest.raises(ValueError):
        gpu_lib.bundle_edges(fn, "WT", layout, initial_bandwidth=0.2)
