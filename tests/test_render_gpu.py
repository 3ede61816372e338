"""The rasteriser on the device (nabo_amd/csrc/render.hip) against the yardstick (tests/_render_ref.py): every image byte for
byte.  After the float64 coordinate-to-pixel step, one correctly rounded IEEE operation per step on gfx950, everything is
integer arithmetic, and tests/test_render_cpu.py has checked on the yardstick that no pixel coordinate of these inputs
sits on an integer."""
import numpy as np
import pytest

from nabo_amd import _bundle, _render

import _bundle_case as bc
import _render_case as rc
import _render_ref as rr

pytestmark = pytest.mark.gpu


def u8(*c):
    return np.array(c, dtype=np.uint8)


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype
    assert a.tobytes() == b.tobytes(), "%d of %d values differ, first at %s" % (
        (a != b).sum(), a.size, tuple(int(i) for i in np.argwhere(a != b)[0]))


def check_edges(W, H, off, pts, chunk=None, view=rc.VIEW):
    want = rr.edge_counts(off, pts, W, H, view)
    with _render.Canvas(W, H, view) as cv:
        if chunk:
            cv.set_option("chunk_points", chunk)
        cv.add_polylines(pts, off)
        same(cv.edge_counts(), want)
        assert not cv.node_counts().any()
    return want


def check_nodes(W, H, pos, r16, rgb, chunk=None, view=rc.VIEW):
    cnt, sums = rr.node_layers(pos, r16, rgb, W, H, view)
    with _render.Canvas(W, H, view) as cv:
        if chunk:
            cv.set_option("chunk_points", chunk)
        cv.add_nodes(pos, r16, rgb, units=True)
        same(cv.node_counts(), cnt)
        same(cv.node_sums(), sums)
        assert not cv.edge_counts().any()
    return cnt, sums


@pytest.mark.parametrize("W,H", rc.CANVASES)
def test_segments_in_every_direction(gpu_lib, W, H):
    check_edges(W, H, *rc.octants(W, H))


@pytest.mark.parametrize("W,H", rc.CANVASES)
@pytest.mark.parametrize("E", rc.E_COUNTS)
def test_polylines(gpu_lib, W, H, E):
    off, pts = rc.polylines(E, W, H)
    if E >= 63:
        assert {2, 3} <= set(np.diff(off).tolist()) and np.diff(off).max() > _render.geometry()["edge_group"]
    check_edges(W, H, off, pts)


def test_both_edge_paths_on_the_long_canvas(gpu_lib):
    W, H = rc.LONG_CANVAS
    g = _render.geometry()
    check_edges(W, H, *rc.threshold_segments(g["edge_short_steps"]))
    off, pts = rc.polylines(200, W, H)
    u, v = rr.point_pixels(pts, W, H, rc.VIEW)
    assert np.abs(np.diff(u)).max() > g["edge_short_steps"] > np.abs(np.diff(u)).min()
    check_edges(W, H, off, pts)


def test_chunks_give_the_same_bytes(gpu_lib):
    W, H = rc.CANVASES[0]
    off, pts = rc.polylines(65, W, H, seed=1)
    want = check_edges(W, H, off, pts)
    for chunk in (1, 7, 64, int(off[-1]) - 1):
        same(check_edges(W, H, off, pts, chunk), want)
    pos, r16, rgb = rc.nodes(65, W, H, _render.geometry())
    for chunk in (1, 7, 64):
        check_nodes(W, H, pos, r16, rgb, chunk)


@pytest.mark.parametrize("W,H,clamp", rc.CLIPPED)
def test_clipped_segments(gpu_lib, W, H, clamp):
    off, pts = rc.clipped(W, H, clamp)
    want = check_edges(W, H, off, pts)
    assert want.sum() >= 7


def test_straight_edges_are_two_point_polylines(gpu_lib):
    W, H = 257, 130
    pos, src, dst, _, _ = rc.whole_graph()
    view = rr.default_viewport(pos)
    want = rr.edge_counts(*rr.straight(pos, src, dst), W, H, view)
    with _render.Canvas(W, H, view) as cv:
        for chunk in (None, 1, 7):
            if chunk:
                cv.set_option("chunk_points", chunk)
            cv.clear()
            cv.add_edges(pos, src, dst)
            same(cv.edge_counts(), want)
        cv.add_edges(pos, src[:0], dst[:0])
        same(cv.edge_counts(), want)


def test_one_hot_pixel(gpu_lib):
    W, H = rc.CANVASES[0]
    off, pts = rc.hot_pixel(W, H)
    with _render.Canvas(W, H, rc.VIEW) as cv:
        cv.add_polylines(pts, off)
        img = cv.edge_counts()
    assert img[H // 2, W // 3] == rc.HOT == img.sum()


@pytest.mark.parametrize("W,H", rc.CANVASES)
@pytest.mark.parametrize("n", rc.E_COUNTS)
def test_nodes(gpu_lib, W, H, n):
    g = _render.geometry()
    radii = set(rc.node_radii(g).tolist())
    assert {0, 1, g["node_small_r"], g["node_small_r"] + 1, g["r_max"]} <= radii
    check_nodes(W, H, *rc.nodes(n, W, H, g))


@pytest.mark.parametrize("W,H", rc.BORDER_CANVASES)
def test_discs_cut_by_the_borders(gpu_lib, W, H):
    g = _render.geometry()
    cnt, _ = check_nodes(W, H, *rc.border_nodes(W, H, g))
    assert cnt[0, 0] > 0 and cnt[H - 1, W - 1] > 0 and cnt[0, W - 1] > 0 and cnt[H - 1, 0] > 0
    check_nodes(W, H, *rc.nodes(200, W, H, g))


def test_coincident_nodes(gpu_lib):
    W, H = rc.CANVASES[0]
    pos, r16, rgb = rc.coincident_nodes(W, H)
    cnt, sums = check_nodes(W, H, pos, r16, rgb)
    assert cnt.max() == 1000 and list(sums[H // 3, W // 2]) == list(rgb.astype(np.int64).sum(axis=0))
    with _render.Canvas(W, H, rc.VIEW) as cv:
        cv.add_nodes(pos, r16, rgb, units=True)
        same(cv.compose("k", lut_e=rr.alpha_lut(0.1, 16), lut_n=rr.alpha_lut(0.01, 65536)),
             rr.compose(np.zeros((H, W)), cnt, sums, (0, 0, 0), rr.alpha_lut(0.1, 16), rr.alpha_lut(0.01, 65536)))


@pytest.mark.parametrize("Le,Ln", [(2, 2), (5, 65536), (65536, 5)])
def test_compose(gpu_lib, Le, Ln):
    """counts at 0, 1, L - 1, L and far above L, under tables of length 2 and 65536; nodes over edges, edges alone, nodes alone"""
    W, H = rc.CANVASES[0]
    counts = (1, 4, 5, 50, 0)
    off, pts = rc.stacked_lines(W, H, counts)
    pos, r16, rgb = rc.stacked_nodes(W, H, counts[::-1])
    ce = rr.edge_counts(off, pts, W, H, rc.VIEW)
    cn, sums = rr.node_layers(pos, r16, rgb, W, H, rc.VIEW)
    assert sorted(set(ce.ravel().tolist())) == [0, 1, 4, 5, 50] == sorted(set(cn.ravel().tolist()))
    assert ((ce > 0) & (cn > 0)).any() and ((ce > 0) & (cn == 0)).any() and ((ce == 0) & (cn > 0)).any()
    lut_e, lut_n = rr.alpha_lut(0.3, Le), rr.alpha_lut(0.45, Ln)
    with _render.Canvas(W, H, rc.VIEW) as cv:
        cv.add_nodes(pos, r16, rgb, units=True)
        cv.add_polylines(pts, off)
        same(cv.compose(u8(200, 30, 90), lut_e=lut_e, lut_n=lut_n), rr.compose(ce, cn, sums, (200, 30, 90), lut_e, lut_n))
        same(cv.compose((0.2, 0.3, 1.0), 0.3, 0.45), rr.compose(ce, cn, sums, (51, 77, 255), rr.alpha_lut(0.3, 65536), rr.alpha_lut(0.45, 65536)))
        ms = cv.last_ms()
        assert all(ms[k] > 0 for k in _render.PHASES) and abs(ms["total"] - sum(ms[k] for k in _render.PHASES)) < 1e-6 * ms["total"]


@pytest.fixture(scope="module")
def bundled(gpu_lib):
    """a resident bundle after its run on the small graph of the bundling tests, and its result"""
    pos, src, dst = bc.graph()
    B = _bundle.Bundle(pos, src, dst, accuracy=64)
    B.run()
    yield B, pos, B.result()
    B.close()


@pytest.mark.parametrize("W,H", [(257, 130), (37, 23)])
def test_add_bundle_equals_the_host_route(gpu_lib, bundled, W, H):
    B, pos, (pts, off) = bundled
    assert np.diff(off).max() > _render.geometry()["edge_group"]
    full = rr.default_viewport(pos)
    zoom = (full[0] + 0.4 * (full[1] - full[0]), full[0] + 0.6 * (full[1] - full[0]), full[2] + 0.3 * (full[3] - full[2]), full[3])
    for view in (full, zoom):
        with _render.Canvas(W, H, view) as a, _render.Canvas(W, H, view) as b:
            a.add_polylines(pts, off)
            b.add_bundle(B)
            want = a.edge_counts()
            assert want.sum() > 0
            same(b.edge_counts(), want)
            b.clear()
            b.set_option("chunk_points", 1000)
            b.add_bundle(B)
            same(b.edge_counts(), want)
    # the bundle is left as it was
    again = B.result()
    assert np.array_equal(again[1], off) and again[0].tobytes() == pts.tobytes()


def test_permutation_and_repeatability(gpu_lib):
    W, H = 257, 130
    g = _render.geometry()
    off, pts = rc.polylines(65, W, H)
    pos, r16, rgb = rc.nodes(65, W, H, g)
    rng = np.random.default_rng(3)
    perm, nperm = rng.permutation(65), rng.permutation(65)
    lines = [pts[off[e]:off[e + 1]] for e in perm]
    poff, ppts = rc.pack(lines)
    with _render.Canvas(W, H, rc.VIEW) as a, _render.Canvas(W, H, rc.VIEW) as b:
        a.add_polylines(pts, off)
        a.add_nodes(pos, r16, rgb, units=True)
        first = a.compose(u8(10, 20, 30), 0.2, 0.5)
        b.add_nodes(pos[nperm], r16[nperm], rgb[nperm], units=True)
        b.add_polylines(ppts, poff)
        same(b.compose(u8(10, 20, 30), 0.2, 0.5), first)
        same(b.edge_counts(), a.edge_counts())
        same(b.node_sums(), a.node_sums())
        a.clear()
        assert not a.edge_counts().any() and not a.node_counts().any() and not a.node_sums().any()
        assert not a.compose(u8(10, 20, 30), 0.2, 0.5).any()
        a.add_polylines(pts, off)
        a.add_nodes(pos, r16, rgb, units=True)
        same(a.compose(u8(10, 20, 30), 0.2, 0.5), first)
    same(first, rr.picture(W, H, rc.VIEW, (off, pts), (pos, r16, rgb), (10, 20, 30), 0.2, 0.5))


def test_refusals_on_the_device(gpu_lib):
    with _render.Canvas(8, 8, (0.0, 1.0, 0.0, 1.0)) as cv:
        for off, pts in (([0, 1], [[0.5, 0.5]]), ([1, 3], [[0.1, 0.1]] * 3), ([0, 2], [[0.5, np.nan], [0.1, 0.1]]), ([0, 2, 3], [[0.5, 0.5]] * 3)):
            with pytest.raises(ValueError):
                cv.add_polylines(pts, off)
        with pytest.raises(ValueError):
            cv.add_edges([[0.5, 0.5]], [0], [1])
        with pytest.raises(ValueError):
            cv.add_nodes([[0.5, 0.5]], [_render.geometry()["r_max"] + 1], "k", units=True)
        with pytest.raises(ValueError):
            cv.set_option("chunk_points", 0)
        with pytest.raises(ValueError):
            cv.set_option("no_such", 1)
        with pytest.raises(ValueError):
            cv.add_bundle(None)
        assert not cv.edge_counts().any() and not cv.node_counts().any()
        cv.add_polylines(np.zeros((0, 2)), [0])
        assert not cv.edge_counts().any()


@pytest.mark.parametrize("bundle", [False, True])
def test_render_graph_is_the_yardsticks(gpu_lib, bundle):
    pos, src, dst, radius, rgb = rc.whole_graph()
    params = rc.WHOLE_BUNDLE if bundle else {}
    img, extent = gpu_lib.render_graph(pos, src, dst, node_rgb=rgb, node_radius=radius, bundle=bundle, **rc.WHOLE, **params)
    assert extent == rr.default_viewport(pos)
    same(img, rc.whole_picture(bundle))
    # one colour, one radius, no edges: the nodes alone
    W, H = rc.WHOLE["width"], rc.WHOLE["height"]
    img, _ = gpu_lib.render_graph(pos, [], [], W, H, "steelblue", 1.5, v_alpha=1.0)
    cn, sums = rr.node_layers(pos, 24, _render._rgb8("steelblue"), W, H, extent)
    same(img, rr.compose(np.zeros((H, W)), cn, sums, (0, 0, 0), rr.alpha_lut(0.1, 65536), rr.alpha_lut(1.0, 65536)))


def test_plot_graph_on_a_mapping_file(gpu_lib, golden, tmp_path):
    pytest.importorskip("h5py")
    from _graph_case import build_file
    from nabo_amd._mapping import read_graph_csr
    from nabo_amd._paths import _open_ref
    import h5py
    fn, _, _ = build_file(str(tmp_path), golden("mapping_small"))
    with h5py.File(fn, "r") as h5:
        names, pos, uid = _open_ref(h5, "WT")
        rows, ptr, nbr, w = read_graph_csr(h5[uid + "_graph"], pos)
    rng = np.random.default_rng(11)
    layout = {r: (float(x), float(y)) for r, (x, y) in zip(rows, rng.random((len(rows), 2)) * 50)}
    layout[rows[3]] = None
    clusters = {r: str(i % 4) for i, r in enumerate(rows) if i % 7}
    ids, xy, src, dst = _bundle._ref_edges(rows, pos, ptr, nbr, w, layout, 0)
    vc = gpu_lib.vertex_colors(clusters)
    rgb = np.array([vc.get(names[i], (128 / 255,) * 3) for i in ids])
    want = gpu_lib.render_graph(xy, src, dst, 128, 96, rgb, gpu_lib.vertex_radii(2, width=128), "k", 0.1, 0.6)
    got = gpu_lib.plot_graph(fn, "WT", layout, clusters, width=128, height=96)
    assert got[1] == want[1]
    same(got[0], want[0])
    with gpu_lib.RefGraph(fn, "WT") as g:
        g.layout, g.clusters = layout, clusters
        same(g.render(width=128, height=96)[0], want[0])
    none = gpu_lib.plot_graph(fn, "WT", layout, clusters, width=128, height=96, draw_edges="none")
    same(none[0], gpu_lib.render_graph(xy, [], [], 128, 96, rgb, gpu_lib.vertex_radii(2, width=128), "k", 0.1, 0.6)[0])
    b = gpu_lib.plot_graph(fn, "WT", layout, clusters, width=128, height=96, bundle_edges=True, accuracy=64)
    same(b[0], gpu_lib.render_graph(xy, src, dst, 128, 96, rgb, gpu_lib.vertex_radii(2, width=128), "k", 0.1, 0.6, bundle=True,
                                    initial_bandwidth=0.1, decay=0.7, accuracy=64)[0])
