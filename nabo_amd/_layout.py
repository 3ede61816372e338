"""The reference graph's 2-D layout on the GPU: ForceAtlas2 with the repulsion summed over every pair.

Array / HDF5 restatement of `Graph.set_ref_layout` (nabo/_graph.py:179-237) and of the two layout writers
(`save_layout_as_json`, `save_layout_as_csv`, :523-541).  The reference hands `refG` to `fa2.ForceAtlas2`, a Python
double loop with a Barnes-Hut tree; here `nabo_layout_run` (include/nabo_layout.h, nabo_amd/csrc/layout.hip) sums every
pair exactly on the device, which is what the tree approximates.  include/nabo_layout.h holds the definition; fa2's own
floating-point results are not pinned.
"""
import ctypes as C
import json

import numpy as np

from . import _lib
from ._graphio import Handle, _f64, check_csr as _check_graph, csr_by_node_id, open_ref

PARAMS = {"outbound_attraction_distribution": True, "edge_weight_influence": 1.0, "jitter_tolerance": 1.0,
          "barnes_hut_optimize": True, "barnes_hut_theta": 1.2, "scaling_ratio": 1.0, "strong_gravity_mode": False,
          "gravity": 1.0}
KERNELS = ("pack", "repulsion", "node", "speed", "move")


def geometry(n=1):
    """(i_block, j_tile, n_splits) of the repulsion kernel as built, n_splits for a graph of n nodes; needs no device"""
    a, b, c = C.c_int32(), C.c_int32(), C.c_int32()
    _lib.check(_lib.lib().nabo_layout_geometry(int(n), C.byref(a), C.byref(b), C.byref(c)))
    return int(a.value), int(b.value), int(c.value)


def _check_params(params):
    unknown = sorted(set(params) - set(PARAMS))
    if unknown:
        raise ValueError("ERROR: unknown layout parameter(s): %s" % ", ".join(unknown))
    p = dict(PARAMS, **params)
    for k in ("edge_weight_influence", "jitter_tolerance", "barnes_hut_theta", "scaling_ratio", "gravity"):
        try:
            p[k] = float(p[k])
        except (TypeError, ValueError):
            raise ValueError("ERROR: %s must be a number" % k)
        if not np.isfinite(p[k]):
            raise ValueError("ERROR: %s must be finite" % k)
    return p


class Layout(Handle):
    """A graph and its layout state resident on one device (nabo_layout_create): the handle the tests and
    tools/bench_layout.py step through; `layout_fa2` is the one-call form."""
    _destroy = "nabo_layout_destroy"

    def __init__(self, ptr, nbr, w, device=0, **params):
        self.n, ptr, nbr, w = _check_graph(ptr, nbr, w)
        p = _check_params(params)
        h = C.c_void_p()
        _lib.check(_lib.lib().nabo_layout_create(C.byref(h), int(device), int(self.n), ptr.ctypes.data, nbr.ctypes.data, w.ctypes.data))
        self._h = h
        _lib.check(_lib.lib().nabo_layout_set_params(h, int(bool(p["outbound_attraction_distribution"])), p["edge_weight_influence"],
                                                     p["jitter_tolerance"], p["scaling_ratio"], int(bool(p["strong_gravity_mode"])),
                                                     p["gravity"], p["barnes_hut_theta"]))

    def set_state(self, x, y, dx=None, dy=None, speed=1.0, eff=1.0):
        x, y = _f64(x, "x", self.n), _f64(y, "y", self.n)
        if (dx is None) != (dy is None):
            raise ValueError("ERROR: give both dx and dy or neither")
        if dx is not None:
            dx, dy = _f64(dx, "dx", self.n), _f64(dy, "dy", self.n)
        _lib.check(_lib.lib().nabo_layout_set_state(self._h, x.ctypes.data, y.ctypes.data, None if dx is None else dx.ctypes.data,
                                                    None if dy is None else dy.ctypes.data, float(speed), float(eff)))

    def get_state(self):
        """{"x", "y", "dx", "dy": float64 [n], "speed", "eff"}"""
        a = [np.empty(self.n, dtype=np.float64) for _ in range(4)]
        speed, eff = C.c_double(), C.c_double()
        _lib.check(_lib.lib().nabo_layout_get_state(self._h, a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, a[3].ctypes.data,
                                                    C.byref(speed), C.byref(eff)))
        return {"x": a[0], "y": a[1], "dx": a[2], "dy": a[3], "speed": speed.value, "eff": eff.value}

    def run(self, niter):
        """the iterations that moved the nodes: niter, or fewer when the forces vanished (S == 0 or T == 0)"""
        done = C.c_int64()
        _lib.check(_lib.lib().nabo_layout_run(self._h, int(niter), C.byref(done)))
        return int(done.value)

    def last_forces(self):
        """{"repulsion", "gravity", "attraction": float64 [n, 2], "S", "T"} of the last iteration run"""
        a = [np.empty((self.n, 2), dtype=np.float64) for _ in range(3)]
        st = (C.c_double * 2)()
        _lib.check(_lib.lib().nabo_layout_last_forces(self._h, a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, st))
        return {"repulsion": a[0], "gravity": a[1], "attraction": a[2], "S": st[0], "T": st[1]}

    def last_ms(self):
        """{"pack", "repulsion", "node", "speed", "move": mean ms per iteration over the last `n_timed` iterations of the
        last run, "run": ms of the whole run, "n_timed"}"""
        ms = (C.c_double * 6)()
        nt = C.c_int64()
        _lib.check(_lib.lib().nabo_layout_last_ms(self._h, ms, C.byref(nt)))
        out = dict(zip(KERNELS, ms[:5]))
        out.update(run=ms[5], n_timed=int(nt.value))
        return out


def layout_fa2(ptr, nbr, w, pos0, niter=500, device=0, **params):
    """ForceAtlas2 on the weighted graph a CSR (ptr, nbr, w) describes -- rows in either arc direction; a pair listed more
    than once keeps its last weight, a self-loop counts towards the degree and exerts no force -- from the positions
    pos0 [n, 2], for niter iterations; float64 [n, 2], not rescaled.  `params`: the reference's
    outbound_attraction_distribution, edge_weight_influence, jitter_tolerance, scaling_ratio, strong_gravity_mode and
    gravity; barnes_hut_optimize and barnes_hut_theta are accepted and ignored (every pair is summed).  If the forces
    vanish (S == 0 or T == 0, where the reference raises ZeroDivisionError) the run ends early with the positions it has."""
    n, ptr, nbr, w = _check_graph(ptr, nbr, w)
    _check_params(params)
    try:
        pos0 = np.asarray(pos0, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("ERROR: pos0 must be numeric")
    if int(niter) < 0:
        raise ValueError("ERROR: niter must not be negative")
    if pos0.ndim != 2 or pos0.shape != (n, 2):
        raise ValueError("ERROR: pos0 must be [n_nodes, 2] = [%d, 2]" % n)
    if not np.isfinite(pos0).all():
        raise ValueError("ERROR: pos0 holds a value that is not finite")
    with Layout(ptr, nbr, w, device, **params) as L:
        L.set_state(pos0[:, 0], pos0[:, 1])
        L.run(niter)
        s = L.get_state()
    return np.stack([s["x"], s["y"]], axis=1)


def _layout_of_graph(ref_nodes, pos, n_ref, rows, ptr, nbr, w, niter, init_pos, seed, disable_rescaling, device, params):
    """rows: the node names of the CSR's rows; pos: name -> node id; ref_nodes: the order of the result"""
    if init_pos is None:
        p0 = np.random.default_rng(seed).random((len(ref_nodes), 2))
    else:
        missing = [x for x in ref_nodes if x not in init_pos]
        if missing:
            raise ValueError("ERROR: init_pos names %d of the %d reference nodes; the first one missing is %s"
                             % (len(ref_nodes) - len(missing), len(ref_nodes), missing[0]))
        try:
            p0 = np.array([[float(init_pos[x][0]), float(init_pos[x][1])] for x in ref_nodes], dtype=np.float64)
        except (TypeError, ValueError, IndexError):
            raise ValueError("ERROR: every value of init_pos must be an (x, y) pair of numbers")
    cptr, cnbr, cw = csr_by_node_id(rows, pos, n_ref, ptr, nbr, w)
    ids = np.array([pos[x] for x in ref_nodes], dtype=np.int64)
    full = np.zeros((n_ref, 2), dtype=np.float64)
    full[ids] = p0
    out = layout_fa2(cptr, cnbr, cw, full, niter, device, **params)[ids]
    if not disable_rescaling:
        out = out - out.min(axis=0)
    return {x: (float(out[i, 0]), float(out[i, 1])) for i, x in enumerate(ref_nodes)}


def _set_ref_layout(mapping_h5_fn, ref_name, niter, init_pos, seed, disable_rescaling, verbose, device, params):
    import h5py
    from ._mapping import read_graph_csr
    params = _check_params(params)
    with h5py.File(mapping_h5_fn, "r") as h5:
        names, pos, ref_uid = open_ref(h5, ref_name)
        rows, ptr, nbr, w = read_graph_csr(h5[ref_uid + "_graph"], pos)
    out = _layout_of_graph(list(rows), pos, len(names), rows, ptr, nbr, w, niter, init_pos, seed, disable_rescaling, device, params)
    if verbose:
        print("ForceAtlas2 layout of %d reference nodes: %d iterations, every pair summed" % (len(out), int(niter)))
    return out


def set_ref_layout(mapping_h5_fn, ref_name, niter=500, init_pos=None, seed=0, disable_rescaling=False,
                   outbound_attraction_distribution=True, edge_weight_influence=1.0, jitter_tolerance=1.0,
                   barnes_hut_optimize=True, barnes_hut_theta=1.2, scaling_ratio=1.0, strong_gravity_mode=False, gravity=1.0,
                   verbose=True, device=0):
    """Graph.set_ref_layout (nabo/_graph.py:179-237) from the mapping file: {reference node: (x, y)} in the reference's
    node order (`refNodes`, the file's), the ForceAtlas2 layout of the reference graph after `niter` iterations, shifted
    so that both coordinates start at 0 unless disable_rescaling.

    What differs from the reference, which calls fa2.ForceAtlas2: the repulsion is the exact sum over
    every pair, not a Barnes-Hut estimate, so barnes_hut_optimize and barnes_hut_theta are accepted and ignored; pair
    terms are float32; and without init_pos the start is `numpy.random.default_rng(seed).random((n, 2))`, one row per
    node in `refNodes` order, where the reference draws unseeded `random.random()` -- the same call gives the same
    layout, bit for bit, every time.  init_pos: {node: (x, y)} that must name every reference node, else ValueError.
    If the forces vanish (the reference: ZeroDivisionError) the positions reached so far are returned."""
    params = dict(outbound_attraction_distribution=outbound_attraction_distribution, edge_weight_influence=edge_weight_influence,
                  jitter_tolerance=jitter_tolerance, barnes_hut_optimize=barnes_hut_optimize, barnes_hut_theta=barnes_hut_theta,
                  scaling_ratio=scaling_ratio, strong_gravity_mode=strong_gravity_mode, gravity=gravity)
    return _set_ref_layout(mapping_h5_fn, ref_name, niter, init_pos, seed, disable_rescaling, verbose, device, params)


def save_layout_as_json(layout, out_fn):
    """Graph.save_layout_as_json (nabo/_graph.py:523-531): what Graph.import_layout_from_json reads"""
    with open(out_fn, "w") as out:
        json.dump({k: (None if v is None else [float(v[0]), float(v[1])]) for k, v in layout.items()}, out, indent=2)


def save_layout_as_csv(layout, out_fn):
    """Graph.save_layout_as_csv (nabo/_graph.py:533-541; `pd.DataFrame(layout).T.to_csv(out_fn, header=None)`): one line
    `node,x,y` per node, no header, floats in their shortest form that reads back to the same value -- what
    Graph.import_layout_from_csv reads with its defaults."""
    with open(out_fn, "w") as out:
        for k, v in layout.items():
            k = str(k)
            if any(c in k for c in ',"\n\r'):
                k = '"' + k.replace('"', '""') + '"'
            out.write("%s,%s,%s\n" % (k, repr(float(v[0])), repr(float(v[1]))))
