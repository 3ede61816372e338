"""The rasteriser (include/nabo_render.h, nabo_amd/_render.py) without a GPU: the header and its symbols, the yardstick
(tests/_render_ref.py) checked by hand, the host-side entry points through ctypes, the wrapper's validation, the colour and
size rules, and the condition on the GPU tests' inputs that no pixel coordinate sits within 1e-9 of an integer."""
import os
import re

import numpy as np
import pytest

import nabo_amd
from nabo_amd import _lib, _render

import _render_case as rc
import _render_ref as rr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 1e-9


def test_public_names_and_symbols():
    for n in ("Canvas", "render_graph", "plot_graph", "draw_image", "vertex_colors", "vertex_radii", "centroid_labels", "alpha_lut",
              "default_viewport"):
        assert n in nabo_amd.__all__ and callable(getattr(nabo_amd, n))
    assert callable(nabo_amd.RefGraph.render)
    src = open(os.path.join(REPO, "include", "nabo_render.h")).read()
    assert '#include "nabo_knn.h"' in src and '#include "nabo_bundle.h"' in src
    assert "nabo_render" not in open(os.path.join(REPO, "include", "nabo_knn.h")).read()
    assert "nabo_render" not in open(os.path.join(REPO, "include", "nabo_bundle.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert sorted(set(re.findall(r"\b(nabo_[a-z0-9_]+)\s*\(", src))) == sorted(_lib.RENDER_SYMBOLS)
    others = (_lib.SYMBOLS + _lib.GRAPH_SYMBOLS + _lib.CLUSTER_SYMBOLS + _lib.DE_SYMBOLS + _lib.PCA_SYMBOLS + _lib.PCA_FIT_SYMBOLS
              + _lib.QC_SYMBOLS + _lib.LAYOUT_SYMBOLS + _lib.UMAP_SYMBOLS + _lib.UMAP_TRANSFORM_SYMBOLS + _lib.COMMUNITY_SYMBOLS
              + _lib.AGGLOM_SYMBOLS + _lib.POTENTIAL_SYMBOLS + _lib.BUNDLE_SYMBOLS)
    assert not set(_lib.RENDER_SYMBOLS) & set(others)
    L = _lib.lib()
    for n in _lib.RENDER_SYMBOLS:
        assert hasattr(L, n), n


def test_header_is_plain_c(tmp_path):
    import subprocess
    src = tmp_path / "render_check.c"
    src.write_text('#include "nabo_render.h"\nint main(void) { nabo_canvas *c = 0; uint8_t lut[3]; (void)c; '
                   'return nabo_render_alpha_lut(0.5, 3, lut) != 0 || lut[0] != 0 || lut[1] != 128 || lut[2] != 191; }\n')
    exe = str(tmp_path / "render_check")
    cmd = ["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(REPO, "include"), str(src), "-L" + os.path.join(REPO, "nabo_amd"),
           "-lnabo_knn", "-Wl,-rpath," + os.path.join(REPO, "nabo_amd"), "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe]
    _lib.lib()
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0, r.stdout
    assert subprocess.run([exe]).returncode == 0


def test_geometry_matches_the_source():
    g = _render.geometry()
    assert g["subpixel_bits"] == 4 and g["r_max"] == rr.R_MAX >= 16 * 64
    assert g["edge_group"] in (4, 8, 16, 32) and g["node_group"] in (4, 8, 16, 32)
    assert g["edge_group"] <= g["edge_short_steps"] < 1024 and 16 < g["node_small_r"] < g["r_max"]
    hip = open(os.path.join(REPO, "nabo_amd", "csrc", "render.hip")).read()
    assert "RND_SUB_BITS = 4, RND_R_MAX = %d;" % g["r_max"] in hip
    assert "RND_EDGE_G = %d, RND_EDGE_SHORT = %d;" % (g["edge_group"], g["edge_short_steps"]) in hip
    assert "RND_NODE_G = %d, RND_NODE_SMALL_R = %d;" % (g["node_group"], g["node_small_r"]) in hip


def test_a_segment_by_hand():
    want = [(0, 0), (1, 0), (2, 1), (3, 1), (4, 2), (5, 2)]
    assert rr.segment_pixels(0, 0, 5, 2) == want
    assert sorted(rr.segment_pixels(5, 2, 0, 0)) == want
    # s + 1 distinct, 8-connected pixels from end to end, whatever the direction
    for u1, v1 in ((7, 3), (-7, 3), (3, -7), (-3, -7), (6, 6), (-6, 6), (0, 5), (-5, 0), (1000, -999)):
        px = rr.segment_pixels(2, -1, 2 + u1, -1 + v1)
        s = max(abs(u1), abs(v1))
        assert len(set(px)) == s + 1 and px[0] == (2, -1) and px[-1] == (2 + u1, -1 + v1)
        assert all(max(abs(a[0] - b[0]), abs(a[1] - b[1])) == 1 for a, b in zip(px, px[1:]))
    view = (0.0, 8.0, 0.0, 4.0)
    img = rr.edge_counts([0, 2], [[0.5, 0.5], [5.5, 2.5]], 8, 4, view)
    assert img.dtype == np.uint32 and img.shape == (4, 8) and img.sum() == 6 and all(img[v, u] == 1 for u, v in want)
    # a three-point polyline counts its joint once; a zero-length polyline counts 1; what leaves the canvas adds nothing
    img = rr.edge_counts([0, 3], [[0.5, 0.5], [3.5, 0.5], [3.5, 3.5]], 8, 4, view)
    assert img.sum() == 7 and img[0, 3] == 1 and img[3, 3] == 1 and img[0, 0] == 1
    assert rr.edge_counts([0, 2], [[2.5, 1.5], [2.6, 1.4]], 8, 4, view).sum() == 1
    assert rr.edge_counts([0, 2, 4], [[2.5, 1.5], [2.5, 1.5], [2.2, 1.2], [2.9, 1.9]], 8, 4, view)[1, 2] == 2
    img = rr.edge_counts([0, 2], [[6.5, 1.5], [11.5, 1.5]], 8, 4, view)
    assert img.sum() == 2 and img[1, 6] == 1 and img[1, 7] == 1
    # row 0 is the lowest y, and the clamp holds far points at +-2^20
    assert rr.edge_counts([0, 2], [[0.5, 0.1], [0.5, 0.2]], 8, 4, view)[0, 0] == 1
    u, v = rr.point_pixels([[1e30, -1e30]], 8, 4, view)
    assert u[0] == 2 ** 20 and v[0] == -2 ** 20


def test_a_disc_by_hand():
    for R, want in ((0, 1), (8, 1), (12, 1), (16, 3), (24, 8), (40, 20)):
        assert len(rr.disc_pixels(100, 100, R)) == want, R
    assert rr.disc_pixels(100, 100, 0) == [(6, 6)] and rr.disc_pixels(-1, -17, 0) == [(-1, -2)]
    # a disc centred on a pixel centre with a radius of exactly one pixel covers the plus of five pixels
    assert rr.disc_pixels(16 * 3 + 8, 16 * 2 + 8, 16) == [(2, 2), (3, 1), (3, 2), (3, 3), (4, 2)]
    view = (0.0, 8.0, 0.0, 4.0)
    cnt, sums = rr.node_layers([[3.5, 2.5], [3.5, 2.5], [100.0, 100.0]], [16, 0, 40], [[10, 20, 30], [1, 2, 3], [9, 9, 9]], 8, 4, view)
    assert cnt.sum() == 6 and cnt[2, 3] == 2 and list(sums[2, 3]) == [11, 22, 33] and list(sums[1, 3]) == [10, 20, 30]
    # cut by the border: only the part inside counts
    cnt, _ = rr.node_layers([[0.5, 0.5]], [16], [[1, 1, 1]], 8, 4, view)
    assert cnt.sum() == 3 and cnt[0, 0] == 1 and cnt[0, 1] == 1 and cnt[1, 0] == 1


@pytest.mark.parametrize("L", [2, 3, 300, 65536])
def test_alpha_tables(L):
    assert not rr.alpha_lut(0.0, L).any() and np.array_equal(_render.alpha_lut(0.0, L), rr.alpha_lut(0.0, L))
    one = _render.alpha_lut(1.0, L)
    assert one[0] == 0 and (one[1:] == 255).all()
    for alpha in (0.1, 0.6, 0.003):
        lut = _render.alpha_lut(alpha, L)
        assert lut.dtype == np.uint8 and lut.shape == (L,) and np.array_equal(lut, rr.alpha_lut(alpha, L))
        assert lut[0] == 0 and lut[1] == int(np.floor(255 * (1 - (1 - alpha)) + 0.5)) and (np.diff(lut.astype(int)) >= 0).all()
        c = np.arange(min(L, 50))
        assert np.abs(lut[:len(c)] - 255 * (1 - (1 - alpha) ** c)).max() <= 0.5 + 1e-9


def test_alpha_table_validation():
    for bad in ((-0.1, 4), (1.1, 4), (float("nan"), 4), (0.5, 1), (0.5, 65537), ("x", 4)):
        with pytest.raises(ValueError):
            _render.alpha_lut(*bad)
    assert _lib.lib().nabo_render_alpha_lut(0.5, 4, None) == _lib.E_INVALID


def test_compose_by_hand():
    lut_e, lut_n = rr.alpha_lut(0.5, 8), rr.alpha_lut(1.0, 8)
    z = np.zeros((1, 1), dtype=np.uint32)
    assert list(rr.compose(z, z, np.zeros((1, 1, 3)), (9, 9, 9), lut_e, lut_n)[0, 0]) == [0, 0, 0, 0]
    # a node-only pixel with An = 255: the mean colour, rounded to nearest (5 / 2 -> 3, 7 / 2 -> 4, 200 / 2 = 100)
    out = rr.compose(z, z + 2, np.array([[[5, 7, 200]]]), (9, 9, 9), lut_e, lut_n)
    assert list(out[0, 0]) == [3, 4, 100, 255]
    # edges alone: the edge colour at the table's opacity
    assert list(rr.compose(z + 1, z, np.zeros((1, 1, 3)), (9, 90, 255), lut_e, lut_n)[0, 0]) == [9, 90, 255, 128]
    # mixed, by hand: Ae = lut(0.5)[2] = 191, An = lut(0.25)[1] = 64, Cn = (100, 0, 50), Ce = (0, 200, 50):
    # t = 191 * 191 = 36481, den = 255 * 64 + 36481 = 52801, A = (52801 + 127) / 255 = 207,
    # C = ((16320 * 100 + 26400) / 52801, (36481 * 200 + 26400) / 52801, (16320 * 50 + 36481 * 50 + 26400) / 52801)
    out = rr.compose(z + 2, z + 1, np.array([[[100, 0, 50]]]), (0, 200, 50), lut_e, rr.alpha_lut(0.25, 8))
    assert lut_e[2] == 191 and rr.alpha_lut(0.25, 8)[1] == 64
    assert list(out[0, 0]) == [1658400 // 52801, 7322600 // 52801, 2666450 // 52801, 207] == [31, 138, 50, 207]
    # counts beyond the table take its last entry
    assert rr.compose(z + 1000, z, np.zeros((1, 1, 3)), (1, 1, 1), lut_e, lut_n)[0, 0, 3] == lut_e[7]


def _point_margins(m, pts, W, H, view=rc.VIEW):
    rr.point_pixels(pts, W, H, view, m)


def test_no_pixel_coordinate_of_the_gpu_cases_sits_on_an_integer():
    """a condition on the GPU tests' inputs, checked on the yardstick alone: a miss means another seed, never an excuse"""
    g = _render.geometry()
    m = {}
    for W, H in rc.CANVASES:
        _point_margins(m, rc.octants(W, H)[1], W, H)
        for E in rc.E_COUNTS:
            _point_margins(m, rc.polylines(E, W, H)[1], W, H)
        for n in rc.E_COUNTS:
            _point_margins(m, rc.nodes(n, W, H, g)[0], W, H)
    for W, H, clamp in rc.CLIPPED:
        _point_margins(m, rc.clipped(W, H, clamp)[1], W, H)
    for W, H in rc.BORDER_CANVASES:
        _point_margins(m, rc.border_nodes(W, H, g)[0], W, H)
        _point_margins(m, rc.nodes(200, W, H, g)[0], W, H)
    W, H = rc.LONG_CANVAS
    _point_margins(m, rc.threshold_segments(g["edge_short_steps"])[1], W, H)
    _point_margins(m, rc.polylines(200, W, H)[1], W, H)
    W, H = rc.CANVASES[0]
    _point_margins(m, rc.hot_pixel(W, H)[1], W, H)
    _point_margins(m, rc.coincident_nodes(W, H)[0], W, H)
    _point_margins(m, rc.stacked_lines(W, H, (1, 4, 5, 50))[1], W, H)
    _point_margins(m, rc.stacked_nodes(W, H, (1, 4, 5, 50))[0], W, H)
    _point_margins(m, rc.polylines(65, W, H, seed=1)[1], W, H)
    assert m["pixel"] > EPS and m["subpixel"] > EPS, m
    # the cases are what they say: the threshold case straddles the threshold, the clipped one reaches the clamp
    off, pts = rc.threshold_segments(g["edge_short_steps"])
    u, v = rr.point_pixels(pts, *rc.LONG_CANVAS, rc.VIEW)
    s = np.maximum(np.abs(np.diff(u)), np.abs(np.diff(v)))[np.setdiff1d(np.arange(len(u) - 1), off[1:-1] - 1)]
    assert {g["edge_short_steps"] - 1, g["edge_short_steps"], g["edge_short_steps"] + 1} <= set(s.tolist())
    u, v = rr.point_pixels(rc.clipped(37, 23)[1], 37, 23, rc.VIEW)
    assert abs(u).max() == 2 ** 20 and abs(v).max() == 2 ** 20 and (abs(u) < 2 ** 20).any()
    assert np.array_equal(rr.edge_counts(*rc.hot_pixel(37, 23), 37, 23, rc.VIEW).ravel().nonzero()[0], [(23 // 2) * 37 + 37 // 3])


def test_no_decision_of_the_whole_call_sits_on_a_threshold():
    off, pts, bm = rc.whole_bundled()
    assert bm["m"] > EPS and bm["pixel"] > EPS and bm["j"] > EPS, bm
    assert np.diff(off).max() > 8, "the bundled case must hold polylines longer than a short group"
    m = {}
    a, b = rc.whole_picture(False, m), rc.whole_picture(True, m)
    assert m["pixel"] > EPS and m["subpixel"] > EPS, m
    assert a.shape == (130, 257, 4) and a.dtype == np.uint8 and not np.array_equal(a, b) and (a[..., 3] > 0).mean() > 0.1


def test_default_viewport():
    assert _render.default_viewport([[0.0, 1.0], [10.0, 1.0]]) == (-0.5, 10.5, 0.5, 1.5)
    pos = rc.whole_graph()[0]
    assert _render.default_viewport(pos) == rr.default_viewport(pos)
    for bad in (np.zeros((0, 2)), [[0.0, np.nan]], [1.0, 2.0]):
        with pytest.raises(ValueError):
            _render.default_viewport(bad)


def test_validation():
    view = (0.0, 1.0, 0.0, 1.0)
    for bad in ((0, 5, view), (5, 8193, view), ("x", 5, view), (5, 5, (0, 0, 0, 1)), (5, 5, (0, 1, 2, 1)), (5, 5, (0, 1, 0)),
                (5, 5, (0, np.inf, 0, 1)), (5, 5, (-1e308, 1e308, 0, 1)), (5, 5, None)):
        with pytest.raises(ValueError):
            nabo_amd.Canvas(*bad)
    pos = np.array([[0.0, 0.0], [1.0, 2.0], [3.0, 1.0]])
    for bad in (dict(width=0), dict(height=9000), dict(viewport=(1, 0, 0, 1)), dict(e_alpha=1.5), dict(v_alpha=-0.1),
                dict(node_radius=-1.0), dict(node_radius=65.0), dict(node_radius=[1.0, 2.0]), dict(node_radius=float("nan")),
                dict(node_rgb="no such colour"), dict(node_rgb=(0.5, 0.5)), dict(node_rgb=(0.5, 0.5, 1.5)), dict(edge_rgb=(2.0, 0, 0)),
                dict(node_rgb=np.zeros((2, 3))), dict(accuracy=64), dict(bundle=True, no_such=1), dict(bundle=True, accuracy=1)):
        with pytest.raises(ValueError):
            nabo_amd.render_graph(pos, [0], [1], **dict(dict(width=16, height=16), **bad))
    for args in ((np.array([[0.0, np.inf], [1.0, 1.0]]), [0], [1]), (pos, [0], [3]), (pos, [-1], [1]), (pos, [0, 1], [1]), (pos[:, :1], [0], [1]),
                 (np.zeros((0, 2)), [], [])):
        with pytest.raises(ValueError):
            nabo_amd.render_graph(*args, width=16, height=16)
    with pytest.raises(ValueError):
        nabo_amd.render_graph(pos, [], [], width=16, height=16, bundle=True)
    assert _render.radius_units([0, 1 / 16, 1.0, 64.0]).tolist() == [0, 1, 16, 1024] and _render.radius_units(0.03) == 0
    assert _render._rgb8("k").tolist() == [0, 0, 0] and _render._rgb8((1.0, 0.5, 0.0)).tolist() == [255, 128, 0]
    assert _render._rgb8(np.array([1, 2, 3], dtype=np.uint8)).tolist() == [1, 2, 3]
    # valid arguments reach the library, which has no device here or runs
    try:
        img, extent = nabo_amd.render_graph(pos, [0, 1], [1, 2], width=16, height=9)
        assert img.shape == (9, 16, 4) and img.dtype == np.uint8 and extent == _render.default_viewport(pos)
    except nabo_amd.NaboError as e:
        assert nabo_amd.device_count() == 0 and "no HIP device" in str(e)


def test_vertex_colors():
    vc = nabo_amd.vertex_colors({"a": "c1", "b": "c10", "c": "c2", "d": "", "e": None, "f": "c10"})
    assert set(vc) == {"a", "b", "c", "f"} and vc["b"] == vc["f"] and len({vc["a"], vc["b"], vc["c"]}) == 3
    # natural order c1 < c2 < c10, the hls palette of three colours from colorsys
    import colorsys
    want = [colorsys.hls_to_rgb(h, 0.6, 0.65) for h in (0.01, 0.01 + 1 / 3, 0.01 + 2 / 3)]
    assert np.allclose([vc["a"], vc["c"], vc["b"]], want, atol=1e-12)
    # numbers: clamped, then binned by digitize over linspace(min, max + 1, n + 1)
    num = nabo_amd.vertex_colors({"a": 1.0, "b": 2.5, "c": 9.0, "d": 100.0}, cmap="viridis", vc_max=9.0)
    assert num["a"] == num["b"] != num["c"] and num["c"] == num["d"]
    import matplotlib
    assert np.allclose(num["a"], matplotlib.colormaps["viridis"](0.25)[:3]) and np.allclose(num["c"], matplotlib.colormaps["viridis"](0.75)[:3])
    ints = nabo_amd.vertex_colors({i: i for i in range(30)}, max_ncolors=5)
    assert len(set(ints.values())) == 5 and ints[0] == ints[5] != ints[7]
    assert np.allclose(ints[0], matplotlib.colormaps["magma_r"](1 / 6)[:3])
    trimmed = nabo_amd.vertex_colors({i: float(i) for i in range(101)}, vc_percent_trim=10, max_ncolors=3)
    assert trimmed[0] == trimmed[10] and trimmed[100] == trimmed[90] and trimmed[0] != trimmed[100]
    # RGB tuples pass; a mixture takes the default colour
    assert nabo_amd.vertex_colors({"a": (0.1, 0.2, 0.3)}) == {"a": (0.1, 0.2, 0.3)}
    assert nabo_amd.vertex_colors({"a": 1, "b": 2.0}, default="red") == {"a": (1.0, 0.0, 0.0), "b": (1.0, 0.0, 0.0)}
    assert nabo_amd.vertex_colors({}) == {} and nabo_amd.vertex_colors({"a": None}) == {}


def test_vertex_radii():
    # s = 2 * 15 points^2 on a 2048-pixel canvas for 5 inches: sqrt(30) / 2 points of 2048 / 360 pixels
    assert abs(nabo_amd.vertex_radii(2) - np.sqrt(30) / 2 * 2048 / 360) < 1e-12
    assert abs(nabo_amd.vertex_radii(2, width=360, fig_size=(5, 5)) - np.sqrt(30) / 2) < 1e-12
    r = nabo_amd.vertex_radii({"a": 1, "b": 4, "c": 16}, vs_scale=1, width=720, fig_size=(10, 3))
    assert np.allclose([r["a"], r["b"], r["c"]], [0.5, 1.0, 2.0])
    r = nabo_amd.vertex_radii({"a": 1.0, "b": 4.0, "c": 16.0}, vs_scale=1, width=720, fig_size=(10, 3), vs_min=4, vs_max=9)
    assert np.allclose([r["a"], r["b"], r["c"]], [1.0, 1.0, 1.5])
    assert nabo_amd.vertex_radii(1e9) == 64.0 and nabo_amd.vertex_radii({}) == {}
    for bad in ("big", None, {"a": "x"}, True):
        with pytest.raises(ValueError):
            nabo_amd.vertex_radii(bad)


def test_node_arrays_follow_plot_nodes():
    names = ["n1", "n2", "n3"]
    args = ("hls", "grey", None, None, None, 40)
    rgb, r = _render._node_arrays(names, "steelblue", None, *args, {"n1": 1, "n2": 4}, 1, None, None, 0, (10, 3), 720)
    assert rgb.tolist() == [_render._rgb8("steelblue").tolist()] * 3 and np.allclose(r, [0.5, 1.0, 0.5])
    # a node the attribute misses takes the default colour; clusters are categories
    rgb, r = _render._node_arrays(names, "steelblue", {"n1": "1", "n3": "2"}, *args, 2, 15, None, None, 0, (5, 5), 2048)
    assert rgb[1].tolist() == _render._rgb8("grey").tolist() and rgb[0].tolist() != rgb[2].tolist() and len(set(r)) == 1
    rgb, _ = _render._node_arrays(names, {"n1": "red", "n2": "blue"}, None, *args, 2, 15, None, None, 0, (5, 5), 2048)
    assert rgb.tolist() == [[255, 0, 0], [0, 0, 255], _render._rgb8("grey").tolist()]
    assert nabo_amd.centroid_labels({"a": (0, 0), "b": (2, 4), "c": None, "d": [1, 1]}, {"a": "x", "b": "x", "c": "x", "d": "y"}) == \
        {"x": (1.0, 2.0), "y": (1.0, 1.0)}


def test_draw_image_puts_text_on_top():
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    fig, ax = plt.subplots(1, 1, figsize=(2, 2))
    try:
        im = nabo_amd.draw_image(ax, np.zeros((9, 16, 4), dtype=np.uint8), (0.0, 4.0, 1.0, 2.0), {"c1": (1.0, 1.5)}, "title")
        assert im.get_extent() == [0.0, 4.0, 1.0, 2.0] and im.origin == "lower"
        assert [t.get_text() for t in ax.texts] == ["c1"] and ax.get_title() == "title"
    finally:
        plt.close(fig)


def test_plot_graph_on_a_mapping_file(golden, tmp_path):
    """the file-level call's argument checks; tests/test_render_gpu.py draws the file on a device"""
    pytest.importorskip("h5py")
    from _graph_case import build_file
    fn, _, _ = build_file(str(tmp_path), golden("mapping_small"))
    with pytest.raises(ValueError):
        nabo_amd.plot_graph(fn, "WT", {}, draw_edges="all")
    with pytest.raises(ValueError):
        nabo_amd.plot_graph(fn, "WT", {}, initial_bandwidth=0.1)
    with pytest.raises(KeyError):
        nabo_amd.plot_graph(fn, "KO", {})
    with pytest.raises(ValueError):
        nabo_amd.plot_graph(fn, "WT", {})          # no node has a position
    with nabo_amd.RefGraph(fn, "WT") as g:
        with pytest.raises(ValueError):
            g.render()                              # no layout yet
