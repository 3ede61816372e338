"""The reference graph drawn on the GPU: nodes and edges aggregated into integer images on the device and composed to one
uint8 [H, W, 4] picture.

Array / HDF5 restatement of the drawing of `GraphPlot` (nabo/_graphplot.py): `_plot_edges`' LineCollection / `ax.plot` and
`_plot_nodes`' scatter, which do not come back for a million nodes and eight million polylines.  include/nabo_render.h
holds the definition and says where it departs from matplotlib (a pixel's node colour is the mean of the nodes covering
it, lines are one pixel wide, nothing is anti-aliased); nabo_amd/csrc/render.hip runs it.  Text -- labels, title, legend
-- stays with matplotlib, drawn on top of the image (`draw_image`).  Only the reference graph is drawn: target nodes have
no position in a reference layout.

The colour rule (`vertex_colors`) restates `GraphPlot._set_vertex_color` with matplotlib's colormaps and `colorsys`:
seaborn and natsort, which the reference takes its palettes and its category order from, are not dependencies, so the
colours are NOT pinned to the reference's `finalColors`.
"""
import colorsys
import ctypes as C
import re

import numpy as np

from . import _lib
from ._bundle import Bundle, _check_graph, _check_params, _read_layout, _ref_edges
from ._graphio import Handle

PHASES = ("clear", "edges", "nodes", "compose")
MAX_SIDE = 8192
LUT_LEN = 65536
_GEOMETRY = ("subpixel_bits", "r_max", "edge_short_steps", "edge_group", "node_small_r", "node_group")


def geometry():
    """{"subpixel_bits", "r_max" (1/16 pixel), "edge_short_steps", "edge_group", "node_small_r" (1/16 pixel), "node_group"}
    of the kernels as built; needs no device"""
    v = [C.c_int32() for _ in _GEOMETRY]
    _lib.check(_lib.lib().nabo_render_geometry(*[C.byref(x) for x in v]))
    return dict(zip(_GEOMETRY, (int(x.value) for x in v)))


def alpha_lut(alpha, length=LUT_LEN):
    """uint8 [length]: the opacity of c strokes of opacity alpha painted over each other, c = 0 .. length - 1 (the table
    `Canvas.compose` takes; include/nabo_render.h).  Needs no device."""
    try:
        alpha, length = float(alpha), int(length)
    except (TypeError, ValueError, OverflowError):
        raise ValueError("ERROR: alpha and length must be numbers")
    if not 0.0 <= alpha <= 1.0:
        raise ValueError("ERROR: alpha must be in [0, 1]")
    if not 2 <= length <= LUT_LEN:
        raise ValueError("ERROR: the length of an alpha table must be in [2, %d]" % LUT_LEN)
    lut = np.empty(length, dtype=np.uint8)
    _lib.check(_lib.lib().nabo_render_alpha_lut(alpha, length, lut.ctypes.data))
    return lut


def _rgb8(c, what="colour"):
    """three uint8 of a matplotlib colour name, a tuple of floats in [0, 1] or three integers 0 .. 255 given as uint8"""
    if isinstance(c, str):
        from matplotlib import colors
        try:
            c = colors.to_rgb(c)
        except ValueError:
            raise ValueError("ERROR: %s: %r is not a colour" % (what, c))
    a = np.asarray(c)
    if a.shape not in ((3,), (4,)):
        raise ValueError("ERROR: %s must be a colour name or an RGB tuple" % what)
    a = a[:3]
    if a.dtype == np.uint8:
        return np.ascontiguousarray(a)
    try:
        a = a.astype(np.float64)
    except (TypeError, ValueError):
        raise ValueError("ERROR: %s must be a colour name or an RGB tuple" % what)
    if not (np.isfinite(a).all() and (a >= 0).all() and (a <= 1).all()):
        raise ValueError("ERROR: %s: float components must be in [0, 1]" % what)
    return np.floor(a * 255 + 0.5).astype(np.uint8)


def _rgb8_rows(rgb, n, what):
    """uint8 [n, 3] of one colour or of n colours (uint8, or floats in [0, 1])"""
    if isinstance(rgb, str):
        return np.ascontiguousarray(np.broadcast_to(_rgb8(rgb, what), (n, 3)))
    a = np.asarray(rgb)
    if a.ndim == 1:
        return np.ascontiguousarray(np.broadcast_to(_rgb8(a, what), (n, 3)))
    if a.shape != (n, 3):
        raise ValueError("ERROR: %s must be one colour or [n_nodes, 3]" % what)
    if a.dtype == np.uint8:
        return np.ascontiguousarray(a)
    try:
        a = a.astype(np.float64)
    except (TypeError, ValueError):
        raise ValueError("ERROR: %s must be numeric" % what)
    if not (np.isfinite(a).all() and (a >= 0).all() and (a <= 1).all()):
        raise ValueError("ERROR: %s: float components must be in [0, 1]" % what)
    return np.floor(a * 255 + 0.5).astype(np.uint8)


def radius_units(radius_px):
    """pixel radii as the canvas takes them: floor(r * 16 + 0.5), uint16, at most R_MAX (64 pixels)"""
    try:
        r = np.asarray(radius_px, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("ERROR: radii must be numbers")
    if not np.isfinite(r).all() or (r < 0).any():
        raise ValueError("ERROR: radii must be finite and not negative")
    u = np.floor(r * 16 + 0.5)
    if u.size and u.max() > geometry()["r_max"]:
        raise ValueError("ERROR: a radius of %g pixels is more than %g" % (r.max(), geometry()["r_max"] / 16))
    return u.astype(np.uint16)


def default_viewport(pos):
    """(x0, x1, y0, y1): the nodes' bounding box widened by 5 % of its extent on each side, or by 0.5 where the extent is 0"""
    pos = np.asarray(pos, dtype=np.float64)
    if pos.ndim != 2 or pos.shape[1] != 2 or pos.shape[0] < 1 or not np.isfinite(pos).all():
        raise ValueError("ERROR: pos must be [n_nodes, 2], finite, with at least one node")
    out = []
    for a in range(2):
        lo, hi = float(pos[:, a].min()), float(pos[:, a].max())
        pad = (hi - lo) * 0.05 if hi > lo else 0.5
        out += [lo - pad, hi + pad]
    return tuple(out)


def _check_viewport(viewport):
    try:
        v = tuple(float(c) for c in viewport)
    except (TypeError, ValueError):
        raise ValueError("ERROR: viewport must be (x0, x1, y0, y1)")
    if len(v) != 4 or not np.isfinite(v).all() or not (v[0] < v[1] and v[2] < v[3]) or not np.isfinite([v[1] - v[0], v[3] - v[2]]).all():
        raise ValueError("ERROR: viewport must be (x0, x1, y0, y1), finite, with x0 < x1 and y0 < y1")
    return v


def _check_size(width, height):
    try:
        width, height = int(width), int(height)
    except (TypeError, ValueError, OverflowError):
        raise ValueError("ERROR: width and height must be integers")
    if not (1 <= width <= MAX_SIDE and 1 <= height <= MAX_SIDE):
        raise ValueError("ERROR: width and height must be in [1, %d]" % MAX_SIDE)
    return width, height


def _check_pos(pos):
    try:
        pos = np.ascontiguousarray(pos, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("ERROR: pos must be numeric")
    if pos.ndim != 2 or pos.shape[1] != 2:
        raise ValueError("ERROR: pos must be [n_nodes, 2]")
    if not np.isfinite(pos).all():
        raise ValueError("ERROR: pos holds a value that is not finite")
    return pos


class Canvas(Handle):
    """A W x H canvas over a viewport, resident on one device (nabo_render_create): edges and nodes are added to its
    integer images in any order and any number of calls, `compose` turns them into the picture, `clear` empties them.
    `render_graph` is the one-call form.  Show the picture with `imshow(image, origin="lower", extent=canvas.viewport)`."""
    _destroy = "nabo_render_destroy"

    def __init__(self, width, height, viewport, device=0):
        self.width, self.height = _check_size(width, height)
        self.viewport = _check_viewport(viewport)
        h = C.c_void_p()
        _lib.check(_lib.lib().nabo_render_create(C.byref(h), int(device), self.width, self.height, *self.viewport))
        self._h = h

    def clear(self):
        _lib.check(_lib.lib().nabo_render_clear(self._h))

    def set_option(self, name, value):
        _lib.check(_lib.lib().nabo_render_set_option(self._h, name.encode("ascii"), int(value)))

    def add_polylines(self, points, offsets):
        """polyline e is points[offsets[e]:offsets[e + 1]], in layout coordinates; what `hammer_bundle` and `Bundle.result`
        return -- one NaN row after each polyline, points [offsets[-1] + n_lines, 2] -- is taken as it is"""
        try:
            off = np.ascontiguousarray(offsets, dtype=np.int64)
            pts = np.ascontiguousarray(points, dtype=np.float64)
        except (TypeError, ValueError, OverflowError):
            raise ValueError("ERROR: points must be numeric and offsets integers")
        if off.ndim != 1 or off.shape[0] < 1 or pts.ndim != 2 or pts.shape[1] != 2:
            raise ValueError("ERROR: offsets must be [n_lines + 1] and points [n_points, 2]")
        n_lines = off.shape[0] - 1
        if n_lines and pts.shape[0] == int(off[-1]) + n_lines and off[0] == 0 and (np.diff(off) >= 0).all():
            keep = np.ones(pts.shape[0], dtype=bool)
            keep[off[1:] + np.arange(n_lines)] = False
            if not np.isnan(pts[~keep]).all():
                raise ValueError("ERROR: points has one row per polyline too many, and they are not NaN rows")
            pts = np.ascontiguousarray(pts[keep])
        if pts.shape[0] != int(off[-1]):
            raise ValueError("ERROR: points must hold offsets[-1] rows")
        _lib.check(_lib.lib().nabo_render_add_polylines(self._h, n_lines, off.ctypes.data, pts.ctypes.data))

    def add_edges(self, pos, src, dst):
        """the straight edges (src[e], dst[e]) of the nodes at pos [n, 2]"""
        pos = _check_pos(pos)
        try:
            src, dst = np.ascontiguousarray(src, dtype=np.int64), np.ascontiguousarray(dst, dtype=np.int64)
        except (TypeError, ValueError, OverflowError):
            raise ValueError("ERROR: src and dst must be integers")
        if src.ndim != 1 or src.shape != dst.shape:
            raise ValueError("ERROR: src and dst must be 1-D and of one length")
        x, y = np.ascontiguousarray(pos[:, 0]), np.ascontiguousarray(pos[:, 1])
        _lib.check(_lib.lib().nabo_render_add_edges(self._h, pos.shape[0], x.ctypes.data, y.ctypes.data, src.shape[0], src.ctypes.data,
                                                    dst.ctypes.data))

    def add_bundle(self, bundle):
        """the polylines a `Bundle` on the same device holds, straight from its device state: the same picture as
        `add_polylines(*bundle.result())` without the points visiting the host"""
        if not isinstance(bundle, Bundle) or bundle._h is None:
            raise ValueError("ERROR: add_bundle takes an open Bundle")
        _lib.check(_lib.lib().nabo_render_add_bundle(self._h, bundle._h))

    def add_nodes(self, pos, radius, rgb, units=False):
        """discs at pos [n, 2]: `radius` in pixels, one number or [n] (with units=True: integers in 1/16 pixel, as the
        C ABI takes them), `rgb` one colour or [n, 3], uint8 or floats in [0, 1]"""
        pos = _check_pos(pos)
        n = pos.shape[0]
        if units:
            r = np.asarray(radius)
            if r.dtype.kind not in "iu" or (r.size and (r.min() < 0 or r.max() > geometry()["r_max"])):
                raise ValueError("ERROR: radii in 1/16 pixel must be integers in [0, %d]" % geometry()["r_max"])
            r = r.astype(np.uint16)
        else:
            r = radius_units(radius)
        if r.ndim == 0:
            r = np.full(n, r, dtype=np.uint16)
        if r.shape != (n,):
            raise ValueError("ERROR: radius must be one number or [n_nodes]")
        r = np.ascontiguousarray(r)
        rgb = _rgb8_rows(rgb, n, "rgb")
        x, y = np.ascontiguousarray(pos[:, 0]), np.ascontiguousarray(pos[:, 1])
        _lib.check(_lib.lib().nabo_render_add_nodes(self._h, n, x.ctypes.data, y.ctypes.data, r.ctypes.data, rgb.ctypes.data))

    def edge_counts(self):
        """uint32 [H, W]: how many polylines' pixels fell on each pixel (row 0 is the lowest y)"""
        img = np.empty((self.height, self.width), dtype=np.uint32)
        _lib.check(_lib.lib().nabo_render_edge_counts(self._h, img.ctypes.data))
        return img

    def node_counts(self):
        """uint32 [H, W]: how many nodes cover each pixel"""
        img = np.empty((self.height, self.width), dtype=np.uint32)
        _lib.check(_lib.lib().nabo_render_node_counts(self._h, img.ctypes.data))
        return img

    def node_sums(self):
        """uint32 [H, W, 3]: the sums of the colour bytes of the nodes covering each pixel"""
        img = np.empty((self.height, self.width, 3), dtype=np.uint32)
        _lib.check(_lib.lib().nabo_render_node_sums(self._h, img.ctypes.data))
        return img

    def compose(self, edge_rgb="k", e_alpha=0.1, v_alpha=0.6, lut_e=None, lut_n=None):
        """uint8 [H, W, 4], RGBA, not premultiplied, nodes over edges over a transparent background.  The alpha tables
        are `alpha_lut(e_alpha)` and `alpha_lut(v_alpha)` unless given (uint8, 2 .. 65536 long)."""
        ce = _rgb8(edge_rgb, "edge_rgb")
        luts = []
        for lut, alpha in ((lut_e, e_alpha), (lut_n, v_alpha)):
            if lut is None:
                lut = alpha_lut(alpha)
            lut = np.ascontiguousarray(lut)
            if lut.dtype != np.uint8 or lut.ndim != 1 or not 2 <= lut.shape[0] <= LUT_LEN:
                raise ValueError("ERROR: an alpha table must be uint8 [2 .. %d]" % LUT_LEN)
            luts.append(lut)
        out = np.empty((self.height, self.width, 4), dtype=np.uint8)
        _lib.check(_lib.lib().nabo_render_compose(self._h, ce.ctypes.data, luts[0].ctypes.data, luts[0].shape[0], luts[1].ctypes.data,
                                                  luts[1].shape[0], out.ctypes.data))
        return out

    def last_ms(self):
        """{"clear", "edges", "nodes", "compose": device ms of the kernels since the last clear, "total": their sum}"""
        ms = (C.c_double * 5)()
        _lib.check(_lib.lib().nabo_render_last_ms(self._h, ms))
        out = dict(zip(PHASES, ms[:4]))
        out["total"] = ms[4]
        return out


def render_graph(pos, src, dst, width=2048, height=2048, node_rgb="steelblue", node_radius=2.0, edge_rgb="k", e_alpha=0.1, v_alpha=0.6,
                 viewport=None, bundle=False, device=0, **bundle_params):
    """The graph of the nodes at pos [n, 2] and the edges (src[e], dst[e]) as one picture: (image uint8 [height, width, 4],
    extent), for `imshow(image, origin="lower", extent=extent)` or `draw_image`.  node_rgb: one colour or [n, 3];
    node_radius: pixels, one number or [n]; no edges (empty src) draws the nodes alone.  viewport: (x0, x1, y0, y1), by
    default `default_viewport(pos)`.  bundle=True bundles the edges first (`Bundle`, with `bundle_params`) and draws them
    from the device where they are."""
    pos = _check_pos(pos)
    if pos.shape[0] < 1:
        raise ValueError("ERROR: there is no node to draw")
    viewport = default_viewport(pos) if viewport is None else _check_viewport(viewport)
    src, dst = np.asarray(src), np.asarray(dst)
    if not bundle and bundle_params:
        raise ValueError("ERROR: bundling parameters are given but bundle is False")
    if src.shape[0] or bundle:
        pos, src, dst = _check_graph(pos, src, dst)
    _check_params(bundle_params)
    # every argument is checked before the device is touched
    width, height = _check_size(width, height)
    radius = radius_units(node_radius)
    if radius.ndim and radius.shape != (pos.shape[0],):
        raise ValueError("ERROR: node_radius must be one number or [n_nodes]")
    node_rgb, edge_rgb = _rgb8_rows(node_rgb, pos.shape[0], "node_rgb"), _rgb8(edge_rgb, "edge_rgb")
    lut_e, lut_n = alpha_lut(e_alpha), alpha_lut(v_alpha)
    with Canvas(width, height, viewport, device) as cv:
        if bundle:
            with Bundle(pos, src, dst, device, **bundle_params) as B:
                B.run()
                cv.add_bundle(B)
        elif src.shape[0]:
            cv.add_edges(pos, src, dst)
        cv.add_nodes(pos, radius, node_rgb, units=True)
        return cv.compose(edge_rgb, lut_e=lut_e, lut_n=lut_n), viewport


def _natural_key(s):
    return [int(t) if t.isdigit() else t for t in re.split(r"(\d+)", s)]


def _palette(cmap, n):
    """n colours: "hls" as seaborn's hls_palette (h = 0.01, l = 0.6, s = 0.65) through colorsys; a listed matplotlib
    colormap of up to 20 colours by its first n (cycled); any other at n points evenly inside (0, 1)"""
    if cmap == "hls":
        hues = np.linspace(0, 1, n + 1)[:-1] + 0.01
        hues = hues % 1
        return [colorsys.hls_to_rgb(float(h), 0.6, 0.65) for h in hues]
    import matplotlib
    from matplotlib import colors
    cm = matplotlib.colormaps[cmap] if isinstance(cmap, str) else cmap
    if isinstance(cm, colors.ListedColormap) and cm.N <= 20:
        return [tuple(cm.colors[i % cm.N][:3]) for i in range(n)]
    return [tuple(float(c) for c in cm(x)[:3]) for x in np.linspace(0, 1, n + 2)[1:-1]]


def vertex_colors(values, cmap=None, default="grey", vc_min=None, vc_max=None, vc_percent_trim=None, max_ncolors=40):
    """{node: (r, g, b) floats}: the rule of `GraphPlot._set_vertex_color` (nabo/_graphplot.py:276-408) for a dict of node
    values.  Values of '' and None are dropped (such a node takes the default colour where the dict is used).  Strings
    are categories, numbered in natural sort order; numbers (all integers or all floats) are clamped to [vc_min, vc_max]
    -- by default the minimum and maximum, with vc_percent_trim the percentiles p and 100 - p -- and binned by
    np.digitize over np.linspace(min, max + 1, n + 1), n = min(distinct values, max_ncolors), into a palette of n
    colours: cmap, by default "hls" below 20 distinct values and "magma_r" from there.  RGB tuples pass as they are.
    Anything else gives every node the default colour.  The palettes are matplotlib's colormaps and colorsys, not
    seaborn's, and the order natural sort, not natsort's: NOT pinned to the reference's finalColors."""
    default = tuple(float(c) / 255 for c in _rgb8(default, "default"))
    vals = {k: v for k, v in dict(values).items() if v is not None and not (isinstance(v, str) and v == "")}
    if not vals:
        return {}
    keys = list(vals)
    v = [vals[k] for k in keys]
    if all(isinstance(x, str) for x in v):
        order = {s: i for i, s in enumerate(sorted(set(v), key=_natural_key))}
        v = [order[x] for x in v]
    if all(isinstance(x, tuple) for x in v):
        if all(len(x) == 3 for x in v):
            return {k: tuple(float(c) for c in x) for k, x in zip(keys, v)}
        return {k: default for k in keys}
    ints = all(isinstance(x, (int, np.integer)) and not isinstance(x, bool) for x in v)
    if not ints and not all(isinstance(x, (float, np.floating)) for x in v):
        return {k: default for k in keys}
    a = np.array(v)
    if vc_min is None:
        vc_min = np.percentile(a, vc_percent_trim) if vc_percent_trim is not None else a.min()
    if vc_max is None:
        vc_max = np.percentile(a, 100 - vc_percent_trim) if vc_percent_trim is not None else a.max()
    a = np.array([vc_max if x > vc_max else vc_min if x < vc_min else x for x in v])
    n_uniq = len(set(a.tolist()))
    if cmap is None:
        cmap = "hls" if n_uniq < 20 else "magma_r"
    n = min(n_uniq, int(max_ncolors))
    pal = _palette(cmap, n)
    bins = np.digitize(a, np.linspace(a.min(), a.max() + 1, n + 1)) - 1
    return {k: tuple(float(c) for c in pal[b]) for k, b in zip(keys, bins)}


def vertex_radii(sizes, vs_scale=15, vs_min=None, vs_max=None, vs_percent_trim=0, fig_size=(5, 5), width=2048):
    """Pixel radii from GraphPlot's vertex sizes (`_set_vertex_size` and `_plot_nodes`, nabo/_graphplot.py:410-456): a number,
    or {node: number} -> {node: radius}.  A node's scatter size is s = size * vs_scale, an area in points^2: a disc of
    diameter sqrt(s) points.  On a canvas `width` pixels wide that stands for fig_size[0] inches a point is
    width / (72 * fig_size[0]) pixels, so radius = sqrt(s) / 2 * width / (72 * fig_size[0]), and at most the canvas's
    64 pixels.  vs_min and vs_max default to the percentiles vs_percent_trim and 100 - vs_percent_trim of the sizes; the
    reference computes them and never applies them, here a size outside them is set to the nearer one."""
    try:
        scale = float(vs_scale) * (float(width) / (72.0 * float(fig_size[0]))) ** 2
    except (TypeError, ValueError, IndexError, ZeroDivisionError):
        raise ValueError("ERROR: vs_scale, width and fig_size must be numbers, fig_size[0] not 0")
    cap = geometry()["r_max"] / 16

    def radius(v):
        return min(float(np.sqrt(max(v, 0) * scale) / 2), cap)
    if not isinstance(sizes, dict):
        if isinstance(sizes, bool) or not isinstance(sizes, (int, float, np.integer, np.floating)):
            raise ValueError("ERROR: Vertex sizes should be float or int values.")
        return radius(sizes)
    if not sizes:
        return {}
    v = np.array(list(sizes.values()))
    if v.dtype.kind not in "iuf" or not np.isfinite(v).all():
        raise ValueError("ERROR: Vertex sizes should be float or int values.")
    lo = np.percentile(v, vs_percent_trim) if vs_min is None else vs_min
    hi = np.percentile(v, 100 - vs_percent_trim) if vs_max is None else vs_max
    return {k: radius(min(max(x, lo), hi)) for k, x in sizes.items()}


def centroid_labels(layout, labels):
    """{label: (x, y)}: the mean position of the nodes that carry each label (GraphPlot's label_attr_type='centroid'), for
    `draw_image`.  labels: {node: label}; nodes without a position are left out."""
    acc = {}
    for node, lab in labels.items():
        p = layout.get(node)
        if p is not None:
            acc.setdefault(lab, []).append((float(p[0]), float(p[1])))
    return {lab: tuple(np.array(p).mean(axis=0)) for lab, p in acc.items()}


def _node_arrays(names, vc, vc_attr, cmap, vc_default, vc_min, vc_max, vc_percent_trim, max_ncolors, vs, vs_scale, vs_min, vs_max,
                 vs_percent_trim, fig_size, width):
    """(rgb uint8 [n, 3], radius float [n]) of the named nodes by GraphPlot's rules: `_plot_nodes` gives a node missing
    from the colour dict the default colour and one missing from the size dict the smallest size"""
    default = tuple(float(c) / 255 for c in _rgb8(vc_default, "vc_default"))
    if vc_attr is not None:
        vc = vertex_colors(vc_attr, cmap, vc_default, vc_min, vc_max, vc_percent_trim, max_ncolors) or vc_default
    elif isinstance(vc, dict):
        v = list(vc.values())
        if v and all(isinstance(x, str) for x in v):   # (a dict of colour names, not of categories)
            vc = {k: tuple(float(c) / 255 for c in _rgb8(x, "vc")) for k, x in vc.items()}
        else:
            vc = vertex_colors(vc, cmap, vc_default, vc_min, vc_max, vc_percent_trim, max_ncolors)
    if isinstance(vc, dict):
        rgb = _rgb8_rows(np.array([vc.get(nm, default) for nm in names], dtype=np.float64).reshape(-1, 3), len(names), "vc")
    else:
        rgb = _rgb8_rows(np.asarray(vc, dtype=np.float64) if isinstance(vc, tuple) else vc, len(names), "vc")
    r = vertex_radii(vs, vs_scale, vs_min, vs_max, vs_percent_trim, fig_size, width)
    if isinstance(r, dict):
        if not r:
            raise ValueError("ERROR: vs is an empty dictionary")
        smallest = min(r.values())
        r = np.array([r.get(nm, smallest) for nm in names], dtype=np.float64)
    else:
        r = np.full(len(names), r, dtype=np.float64)
    return rgb, r


def plot_graph(mapping_h5_fn, ref_name, layout, clusters=None, vc="steelblue", cmap=None, vc_attr=None, vc_default="grey", vec=None,
               vc_min=None, vc_max=None, vc_percent_trim=None, max_ncolors=40, vs=2, vs_scale=15, vs_min=None, vs_max=None,
               vs_percent_trim=0, vlw=0, v_alpha=0.6, v_zorder=None, draw_edges="ref", ec="k", elw=0.1, e_alpha=0.1, bundle_edges=False,
               bundle_bw=0.1, bundle_decay=0.7, edge_min_weight=0, width=2048, height=2048, fig_size=(5, 5), viewport=None, device=0,
               **bundle_params):
    """The picture `GraphPlot(g, only_ref=True, ...)` draws of the reference graph (nabo/_graphplot.py), from the mapping
    file: (image uint8 [height, width, 4], extent), for `draw_image`.  The argument names are GraphPlot's.  `layout`: the
    dict `set_ref_layout` returns, or the JSON / CSV file written from it; the reference nodes with a position are drawn.
    `vc`: a colour, or {node: value / colour name / RGB tuple}; `vc_attr`: {node: attribute value} (GraphPlot reads them
    off the networkx graph), which overrides vc; `clusters`: shorthand for vc_attr, what `make_clusters` returns; the
    colours follow `vertex_colors` and are not pinned to the reference's.  `vs`: a number or {node: number}
    (`vertex_radii`; the canvas stands for a figure fig_size[0] inches wide).  draw_edges: "ref" or "none"; the edges are
    taken by the rule of `bundle_edges` (weight > edge_min_weight, both ends placed) and with bundle_edges=True bundled
    on the device (bundle_bw, bundle_decay, `bundle_params`).  elw, vlw, vec and v_zorder are accepted and ignored: lines
    are one pixel wide, discs have no outline, and a pixel's colour is the mean of the nodes on it."""
    import h5py
    from ._graphio import open_ref
    from ._mapping import read_graph_csr
    if draw_edges not in ("ref", "none"):
        raise ValueError("ERROR: draw_edges must be 'ref' or 'none': only the reference graph has positions")
    if "initial_bandwidth" in bundle_params or "decay" in bundle_params:
        raise ValueError("ERROR: give bundle_bw and bundle_decay, not initial_bandwidth and decay")
    layout = _read_layout(layout)
    with h5py.File(mapping_h5_fn, "r") as h5:
        all_names, pos, ref_uid = open_ref(h5, ref_name)
        rows, ptr, nbr, w = read_graph_csr(h5[ref_uid + "_graph"], pos)
    ids, xy, src, dst = _ref_edges(rows, pos, ptr, nbr, w, layout, edge_min_weight)
    return _plot_arrays([all_names[i] for i in ids], xy, src, dst, clusters, vc, cmap, vc_attr, vc_default, vc_min, vc_max,
                        vc_percent_trim, max_ncolors, vs, vs_scale, vs_min, vs_max, vs_percent_trim, v_alpha, draw_edges, ec, e_alpha,
                        bundle_edges, bundle_bw, bundle_decay, width, height, fig_size, viewport, device, bundle_params)


def _plot_arrays(names, xy, src, dst, clusters, vc, cmap, vc_attr, vc_default, vc_min, vc_max, vc_percent_trim, max_ncolors, vs, vs_scale,
                 vs_min, vs_max, vs_percent_trim, v_alpha, draw_edges, ec, e_alpha, bundle_edges, bundle_bw, bundle_decay, width, height,
                 fig_size, viewport, device, bundle_params):
    """plot_graph once the file is read: the placed nodes' names and positions and the edges between them"""
    if len(names) == 0:
        raise ValueError("ERROR: None of the nodes in the graph has 'pos' attribute")
    if vc_attr is None and clusters is not None:
        vc_attr = clusters
    rgb, radius = _node_arrays(names, vc, vc_attr, cmap, vc_default, vc_min, vc_max, vc_percent_trim, max_ncolors, vs, vs_scale, vs_min,
                               vs_max, vs_percent_trim, fig_size, width)
    if draw_edges == "none" or len(src) == 0:
        src = dst = np.zeros(0, dtype=np.int64)
        bundle_edges = False
    params = dict(bundle_params, initial_bandwidth=bundle_bw, decay=bundle_decay) if bundle_edges else {}
    return render_graph(xy, src, dst, width, height, rgb, radius, ec, e_alpha, v_alpha, viewport, bool(bundle_edges), device, **params)


def draw_image(ax, image, extent, labels=None, title=None, label_fs=16, title_fs=30):
    """Put the picture on a matplotlib axis -- `imshow(image, origin="lower", extent=extent)` -- with GraphPlot's centroid
    labels ({text: (x, y)}, see `centroid_labels`) and title on top, its ticks and spines removed.  Returns the image
    artist.  Text is the one thing matplotlib still draws."""
    im = ax.imshow(image, origin="lower", extent=tuple(extent), aspect="auto", interpolation="nearest")
    for text, (x, y) in (labels or {}).items():
        ax.text(x, y, text, ha="center", fontsize=label_fs)
    if title is not None:
        ax.set_title(title, fontsize=title_fs)
    ax.set_xticklabels([])
    ax.set_yticklabels([])
    for s in ("top", "bottom", "left", "right"):
        ax.spines[s].set_visible(False)
    ax.grid(False)
    return im
