"""Edge bundling on the GPU: the laid-out reference graph's edges drawn together by advection along the gradient of
their own density.

Array / HDF5 restatement of the bundling of `GraphPlot(..., bundle_edges=True)` (nabo/_graphplot.py:192-220), which hands
positions and edges to `datashader.bundling.hammer_bundle`.  include/nabo_bundle.h holds the definition and says where it
departs from datashader, whose own floating-point results are not pinned; nabo_amd/csrc/bundle.hip runs
it.  Only the reference graph is drawn: target nodes have no position in a reference layout.  Drawing: `ax.plot(points[:, 0], points[:, 1])`
for the polylines of a small graph; for graphs too large for that, `Canvas.add_bundle` (nabo_amd/_render.py) rasterises a
resident bundle's polylines on the device.
"""
import ctypes as C
import json

import numpy as np

from . import _lib
from ._graphio import Handle

PARAMS = {"initial_bandwidth": 0.05, "decay": 0.7, "iterations": 4, "accuracy": 500, "advect_iterations": 50,
          "resample_every": 2, "min_segment_length": 0.008, "max_segment_length": 0.016, "tension": 0.3,
          "smooth_passes": 10, "batch_size": 20000}
_INTS = ("iterations", "accuracy", "advect_iterations", "resample_every", "smooth_passes", "batch_size")
PHASES = ("resample", "density", "field", "advect", "smooth")


def geometry():
    """{"p_max", "short_group", "short_cap", "long_group"} of the round kernels as built; needs no device"""
    v = [C.c_int32() for _ in range(4)]
    _lib.check(_lib.lib().nabo_bundle_geometry(*[C.byref(x) for x in v]))
    return dict(zip(("p_max", "short_group", "short_cap", "long_group"), (int(x.value) for x in v)))


def blur_weights(b):
    """the normalised weights w[t + R], t = -R .. R, of a blur of bandwidth b pixels (float64 [2R + 1]); needs no device"""
    R = C.c_int32()
    _lib.check(_lib.lib().nabo_bundle_blur_weights(float(b), C.byref(R), None, 0))
    w = np.empty(2 * R.value + 1, dtype=np.float64)
    _lib.check(_lib.lib().nabo_bundle_blur_weights(float(b), C.byref(R), w.ctypes.data, w.shape[0]))
    return w


def _check_params(params):
    unknown = sorted(set(params) - set(PARAMS))
    if unknown:
        raise ValueError("ERROR: unknown bundling parameter(s): %s" % ", ".join(unknown))
    p = dict(PARAMS, **params)
    for k in PARAMS:
        try:
            p[k] = int(p[k]) if k in _INTS else float(p[k])
        except (TypeError, ValueError, OverflowError):
            raise ValueError("ERROR: %s must be a number" % k)
        if k not in _INTS and not np.isfinite(p[k]):
            raise ValueError("ERROR: %s must be finite" % k)
    if not 2 <= p["accuracy"] <= 4096:
        raise ValueError("ERROR: accuracy must be in [2, 4096]")
    if not 0.0 < p["decay"] <= 1.0:
        raise ValueError("ERROR: decay must be in (0, 1]")
    if not 0.0 <= p["tension"] <= 1.0:
        raise ValueError("ERROR: tension must be in [0, 1]")
    if not 0.0 < p["min_segment_length"] <= p["max_segment_length"]:
        raise ValueError("ERROR: segment lengths must satisfy 0 < min_segment_length <= max_segment_length")
    if p["initial_bandwidth"] <= 0.0:
        raise ValueError("ERROR: initial_bandwidth must be positive")
    if min(p["iterations"], p["advect_iterations"], p["smooth_passes"]) < 0 or p["resample_every"] < 1:
        raise ValueError("ERROR: iterations, advect_iterations and smooth_passes must be >= 0 and resample_every >= 1")
    return p


def _check_graph(pos, src, dst):
    try:
        pos = np.ascontiguousarray(pos, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("ERROR: pos must be numeric")
    if pos.ndim != 2 or pos.shape[1] != 2 or pos.shape[0] < 1:
        raise ValueError("ERROR: pos must be [n_nodes, 2] with at least one node")
    if not np.isfinite(pos).all():
        raise ValueError("ERROR: pos holds a value that is not finite")
    try:
        src, dst = np.ascontiguousarray(src, dtype=np.int64), np.ascontiguousarray(dst, dtype=np.int64)
    except (TypeError, ValueError, OverflowError):
        raise ValueError("ERROR: src and dst must be integers")
    if src.ndim != 1 or src.shape != dst.shape:
        raise ValueError("ERROR: src and dst must be 1-D and of one length")
    if src.shape[0] == 0:
        raise ValueError("ERROR: there is no edge to bundle")
    if min(src.min(), dst.min()) < 0 or max(src.max(), dst.max()) >= pos.shape[0]:
        raise ValueError("ERROR: src or dst holds an entry that is not a node in [0, %d)" % pos.shape[0])
    return pos, src, dst


class Bundle(Handle):
    """Nodes, edges and the edges' polylines resident on one device (nabo_bundle_create): the handle the tests and
    tools/bench_bundle.py step through; `hammer_bundle` is the one-call form.  To show a graph of millions of edges, hand the
    handle to `Canvas.add_bundle`, which draws the polylines as lines; `density()` counts their sample points only."""
    _destroy = "nabo_bundle_destroy"

    def __init__(self, pos, src, dst, device=0, **params):
        pos, src, dst = _check_graph(pos, src, dst)
        self.n, self.n_edges = pos.shape[0], src.shape[0]
        x, y = np.ascontiguousarray(pos[:, 0]), np.ascontiguousarray(pos[:, 1])
        h = C.c_void_p()
        _lib.check(_lib.lib().nabo_bundle_create(C.byref(h), int(device), self.n, x.ctypes.data, y.ctypes.data, self.n_edges,
                                                 src.ctypes.data, dst.ctypes.data))
        self._h = h
        self.set_params(**params)

    def set_params(self, **params):
        p = self.params = _check_params(params)
        _lib.check(_lib.lib().nabo_bundle_set_params(self._h, p["initial_bandwidth"], p["decay"], p["iterations"], p["accuracy"],
                                                     p["advect_iterations"], p["resample_every"], p["min_segment_length"],
                                                     p["max_segment_length"], p["tension"], p["smooth_passes"], p["batch_size"]))

    def set_option(self, name, value):
        _lib.check(_lib.lib().nabo_bundle_set_option(self._h, name.encode("ascii"), int(value)))

    def get_points(self):
        """(offsets int64 [E + 1], normalised points float64 [offsets[E], 2])"""
        n = C.c_int64()
        off = np.empty(self.n_edges + 1, dtype=np.int64)
        _lib.check(_lib.lib().nabo_bundle_get_points(self._h, C.byref(n), off.ctypes.data, None))
        pts = np.empty((n.value, 2), dtype=np.float64)
        _lib.check(_lib.lib().nabo_bundle_get_points(self._h, None, None, pts.ctypes.data))
        return off, pts

    def set_points(self, offsets, points):
        off = np.ascontiguousarray(offsets, dtype=np.int64)
        pts = np.ascontiguousarray(points, dtype=np.float64)
        if off.shape != (self.n_edges + 1,) or pts.ndim != 2 or pts.shape[1] != 2 or pts.shape[0] != int(off[-1]):
            raise ValueError("ERROR: offsets must be [n_edges + 1] and points [offsets[-1], 2]")
        _lib.check(_lib.lib().nabo_bundle_set_points(self._h, off.ctypes.data, pts.ctypes.data))

    def resample(self):
        _lib.check(_lib.lib().nabo_bundle_resample(self._h))

    def density(self):
        """uint32 [A + 1, A + 1]: how many points of the present polylines fall into each pixel"""
        a1 = self.params["accuracy"] + 1
        img = np.empty((a1, a1), dtype=np.uint32)
        _lib.check(_lib.lib().nabo_bundle_density(self._h, img.ctypes.data))
        return img

    def field(self, b):
        """(blurred, GX, GY), float64 [A + 1, A + 1] each, of the last density for a bandwidth of b pixels"""
        a1 = self.params["accuracy"] + 1
        out = [np.empty((a1, a1), dtype=np.float64) for _ in range(3)]
        _lib.check(_lib.lib().nabo_bundle_field(self._h, float(b), out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data))
        return tuple(out)

    def advect(self, n_steps):
        _lib.check(_lib.lib().nabo_bundle_advect(self._h, int(n_steps)))

    def smooth(self, passes):
        _lib.check(_lib.lib().nabo_bundle_smooth(self._h, int(passes)))

    def run(self):
        _lib.check(_lib.lib().nabo_bundle_run(self._h))

    def result(self):
        """(points float64 [offsets[E] + E, 2], de-normalised, one NaN row after each edge; offsets int64 [E + 1])"""
        off = np.empty(self.n_edges + 1, dtype=np.int64)
        _lib.check(_lib.lib().nabo_bundle_result(self._h, off.ctypes.data, None))
        pts = np.empty((int(off[-1]) + self.n_edges, 2), dtype=np.float64)
        _lib.check(_lib.lib().nabo_bundle_result(self._h, None, pts.ctypes.data))
        return pts, off

    def last_ms(self):
        """{"resample", "density", "field", "advect", "smooth": device ms of the last run, "total": their sum}"""
        ms = (C.c_double * 6)()
        _lib.check(_lib.lib().nabo_bundle_last_ms(self._h, ms))
        out = dict(zip(PHASES, ms[:5]))
        out["total"] = ms[5]
        return out


def hammer_bundle(pos, src, dst, device=0, **params):
    """Bundle the edges (src[e], dst[e]) of the nodes at pos [n, 2]: (points, offsets).  Edge e is the polyline
    points[offsets[e] + e : offsets[e + 1] + e], in the coordinates of pos, and a NaN row follows each edge, so that
    `ax.plot(points[:, 0], points[:, 1])` draws them apart.  `params`: datashader's initial_bandwidth, decay, iterations,
    accuracy, advect_iterations, min_segment_length, max_segment_length, tension, and resample_every, smooth_passes;
    batch_size is accepted and ignored.  include/nabo_bundle.h has the definition."""
    _check_params(params)
    with Bundle(pos, src, dst, device, **params) as B:
        B.run()
        return B.result()


def _read_layout(layout):
    if isinstance(layout, dict):
        return layout
    fn = str(layout)
    if fn.lower().endswith(".json"):
        with open(fn) as f:
            return json.load(f)
    import csv
    out = {}
    with open(fn, newline="") as f:
        for row in csv.reader(f):
            if len(row) != 3:
                raise ValueError("ERROR: %s: a layout line must read node,x,y" % fn)
            out[row[0]] = (float(row[1]), float(row[2]))
    return out


def _ref_edges(rows, pos, ptr, nbr, w, layout, edge_min_weight):
    """GraphPlot's draw_edges='ref' rule on the file's rows: every undirected pair once, where the file lists it first,
    with the weight it lists last (networkx's add_edge), kept if that weight is > edge_min_weight and both ends have a
    position.  (node ids with a position, their positions [k, 2], src, dst as indices into those)"""
    names = [None] * len(pos)
    for k, v in pos.items():
        names[v] = k
    a = np.repeat(np.array([pos[r] for r in rows], dtype=np.int64), np.diff(ptr))
    b = np.asarray(nbr, dtype=np.int64)
    key = np.minimum(a, b) * len(pos) + np.maximum(a, b)
    _, first = np.unique(key, return_index=True)
    _, last_rev = np.unique(key[::-1], return_index=True)
    last = key.shape[0] - 1 - last_rev
    order = np.argsort(first, kind="stable")
    first, last = first[order], last[order]
    have = np.array([layout.get(nm) is not None for nm in names], dtype=bool)
    keep = (np.asarray(w)[last] > edge_min_weight) & have[a[first]] & have[b[first]]
    ids = np.flatnonzero(have)
    local = np.full(len(pos), -1, dtype=np.int64)
    local[ids] = np.arange(ids.shape[0])
    try:
        xy = np.array([[float(layout[names[i]][0]), float(layout[names[i]][1])] for i in ids], dtype=np.float64).reshape(-1, 2)
    except (TypeError, ValueError, IndexError):
        raise ValueError("ERROR: every value of the layout must be an (x, y) pair of numbers")
    return ids, xy, local[a[first][keep]], local[b[first][keep]]


def bundle_edges(mapping_h5_fn, ref_name, layout, edge_min_weight=0, bundle_bw=0.1, bundle_decay=0.7, device=0, **params):
    """The bundled edges `GraphPlot(draw_edges='ref', bundle_edges=True)` draws (nabo/_graphplot.py:192-247), from the
    mapping file: (points, offsets) as `hammer_bundle` returns them.  `layout`: the dict `set_ref_layout` returns, or the
    JSON / CSV file `save_layout_as_json` / `save_layout_as_csv` wrote.  Every undirected edge of the reference graph is
    taken once, in the file's order, if its weight is > edge_min_weight and both ends have a position; bundle_bw and
    bundle_decay are hammer_bundle's initial_bandwidth and decay, as in the reference, and `params` its other parameters.
    Unlike the reference, which drops datashader's NaN rows and so joins consecutive edges, the NaN rows stay."""
    import h5py
    from ._graphio import open_ref
    from ._mapping import read_graph_csr
    if "initial_bandwidth" in params or "decay" in params:
        raise ValueError("ERROR: give bundle_bw and bundle_decay, not initial_bandwidth and decay")
    layout = _read_layout(layout)
    with h5py.File(mapping_h5_fn, "r") as h5:
        _, pos, ref_uid = open_ref(h5, ref_name)
        rows, ptr, nbr, w = read_graph_csr(h5[ref_uid + "_graph"], pos)
    _, xy, src, dst = _ref_edges(rows, pos, ptr, nbr, w, layout, edge_min_weight)
    return hammer_bundle(xy, src, dst, device, initial_bandwidth=bundle_bw, decay=bundle_decay, **params)
