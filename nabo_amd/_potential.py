"""Differentiation potential of the reference graph on the GPU: one sparse symmetric solve where the reference takes a
dense pseudo-inverse.

Array / HDF5 restatement of `Graph.calc_diff_potential` (nabo/_graph.py:918-954; the population-balance potential of
Weinreb et al. 2017): V = pinv(I - D^-1 A) r on the unweighted reference graph.  The reference builds the dense n x n
matrix and hands it to numpy.linalg.pinv; here `nabo_potential_solve` (include/nabo_potential.h,
nabo_amd/csrc/potential.hip) solves K x = d * r' by conjugate gradients with the Jacobi preconditioner on the device and
takes the minimum-norm solution per connected component, which is the same vector.
"""
import ctypes as C
import warnings

import numpy as np

from . import _lib
from ._graphio import Handle, _f64, check_csr, read_ref_graph

PHASES = ("prepare", "iterate", "finish", "run")
STATUS = ("running", "converged", "max_iter", "breakdown")


def geometry():
    """(group, long_threshold, block_rows) of the product as built: `group` lanes share a row of at most
    `long_threshold` arcs, a longer row takes a workgroup; a workgroup covers `block_rows` consecutive rows and adds
    their terms of every dot product into one partial sum; needs no device"""
    a, b, c = C.c_int32(), C.c_int32(), C.c_int32()
    _lib.check(_lib.lib().nabo_potential_geometry(C.byref(a), C.byref(b), C.byref(c)))
    return int(a.value), int(b.value), int(c.value)


def _check_graph(ptr, nbr):
    n, ptr, nbr = check_csr(ptr, nbr)
    seen = np.zeros(n, dtype=bool)
    seen[nbr] = True
    seen[np.diff(ptr) > 0] = True
    if not seen.all():
        raise ValueError("ERROR: node %d has no edge: its row of I - A/D is a division by zero" % int(np.flatnonzero(~seen)[0]))
    return n, ptr, nbr


def _check_params(tol, max_iter):
    try:
        tol = float(tol)
    except (TypeError, ValueError):
        raise ValueError("ERROR: tol must be a number")
    if not np.isfinite(tol) or tol < 0:
        raise ValueError("ERROR: tol must be finite and not negative")
    if isinstance(max_iter, bool) or not isinstance(max_iter, (int, np.integer)):
        raise ValueError("ERROR: max_iter must be an integer")
    if max_iter < 1 or max_iter >= 2 ** 63:
        raise ValueError("ERROR: max_iter=%d must be at least 1" % max_iter)
    return tol, int(max_iter)


class Potential(Handle):
    """A graph resident on one device and the state of its solve (nabo_potential_create): the handle the tests and
    tools/bench_potential.py step through; `diff_potential_csr` is the one-call form."""
    _destroy = "nabo_potential_destroy"

    def __init__(self, ptr, nbr, tol=1e-10, max_iter=10000, device=0):
        self.n, ptr, nbr = _check_graph(ptr, nbr)
        p = _check_params(tol, max_iter)
        h = C.c_void_p()
        _lib.check(_lib.lib().nabo_potential_create(C.byref(h), int(device), int(self.n), ptr.ctypes.data, nbr.ctypes.data))
        self._h = h
        self.set_params(*p)

    def set_params(self, tol=1e-10, max_iter=10000):
        self.tol, self.max_iter = _check_params(tol, max_iter)
        _lib.check(_lib.lib().nabo_potential_set_params(self._h, self.tol, self.max_iter))

    def graph_size(self):
        """(n, n_arcs, n_long): nodes, off-diagonal arcs (both directions), rows that take a workgroup"""
        a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
        _lib.check(_lib.lib().nabo_potential_graph_size(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return int(a.value), int(b.value), int(c.value)

    def _r(self, r):
        return None if r is None else _f64(r, "r", self.n)

    def prepare(self, r=None):
        """components, the projected right-hand side b and the start of the iteration; r [n] finite, None = all ones"""
        r = self._r(r)
        _lib.check(_lib.lib().nabo_potential_prepare(self._h, None if r is None else r.ctypes.data))

    def get_prepared(self):
        """{"label": int32 (the smallest node of each node's component), "d", "c": int64, "b": float64}"""
        lab, d, c = np.empty(self.n, dtype=np.int32), np.empty(self.n, dtype=np.int64), np.empty(self.n, dtype=np.int64)
        b = np.empty(self.n, dtype=np.float64)
        _lib.check(_lib.lib().nabo_potential_get_prepared(self._h, lab.ctypes.data, d.ctypes.data, c.ctypes.data, b.ctypes.data))
        return {"label": lab, "d": d, "c": c, "b": b}

    def iterate(self, count=1):
        """up to `count` more iterations; True once the run has stopped"""
        done = C.c_int32()
        _lib.check(_lib.lib().nabo_potential_iterate(self._h, int(count), C.byref(done)))
        return bool(done.value)

    def get_state(self):
        """{"x", "res", "p": float64 [n], "rho", "it"}"""
        x, res, p = (np.empty(self.n, dtype=np.float64) for _ in range(3))
        rho, it = C.c_double(), C.c_int64()
        _lib.check(_lib.lib().nabo_potential_get_state(self._h, x.ctypes.data, res.ctypes.data, p.ctypes.data, C.byref(rho), C.byref(it)))
        return {"x": x, "res": res, "p": p, "rho": rho.value, "it": int(it.value)}

    def set_state(self, x, res, p, rho, it):
        x, res, p = _f64(x, "x", self.n), _f64(res, "res", self.n), _f64(p, "p", self.n)
        _lib.check(_lib.lib().nabo_potential_set_state(self._h, x.ctypes.data, res.ctypes.data, p.ctypes.data, float(rho), int(it)))

    def finish(self):
        """V float64 [n]: the current x less its mean over each component; the true residual goes to info()"""
        V = np.empty(self.n, dtype=np.float64)
        _lib.check(_lib.lib().nabo_potential_finish(self._h, V.ctypes.data))
        return V

    def solve(self, r=None):
        """the whole run: (V float64 [n], info) as diff_potential_csr returns them"""
        r = self._r(r)
        V = np.empty(self.n, dtype=np.float64)
        _lib.check(_lib.lib().nabo_potential_solve(self._h, None if r is None else r.ctypes.data, V.ctypes.data))
        return V, self.info()

    def info(self):
        it, st, nc = C.c_int64(), C.c_int32(), C.c_int64()
        rel, true = C.c_double(), C.c_double()
        _lib.check(_lib.lib().nabo_potential_info(self._h, C.byref(it), C.byref(st), C.byref(rel), C.byref(true), C.byref(nc)))
        return {"iterations": int(it.value), "status": STATUS[st.value], "residual": rel.value, "true_residual": true.value,
                "n_components": int(nc.value), "ms": self.last_ms()}

    def last_ms(self):
        """{"prepare", "iterate", "finish", "run": device ms since the last prepare}"""
        ms = (C.c_double * 4)()
        _lib.check(_lib.lib().nabo_potential_last_ms(self._h, ms))
        return dict(zip(PHASES, ms[:4]))


def diff_potential_csr(ptr, nbr, r=None, tol=1e-10, max_iter=10000, device=0):
    """V = pinv(I - D^-1 A) r on the unweighted graph a CSR (ptr, nbr) describes -- rows in either arc direction, a pair
    listed more than once counts once, a self-loop counts once in its node's degree -- by the solve of
    include/nabo_potential.h.  r: [n] finite, None = all ones.  Returns (V float64 [n], info): info["iterations"],
    "status" ("converged", "max_iter" or "breakdown"), "residual" (the recurrence's, relative to ||b||), "true_residual"
    (||b - K x|| / ||b|| from one more product), "n_components" and "ms".  A node without any edge raises ValueError.  A
    run that ends by max_iter or by a breakdown returns what it has and issues a RuntimeWarning with the true residual.
    The same call gives the same bits every time."""
    if r is not None:
        r = _f64(r, "r", _check_graph(ptr, nbr)[0])
    with Potential(ptr, nbr, tol, max_iter, device) as H:
        V, info = H.solve(r)
    if info["status"] != "converged":
        warnings.warn("the potential's solve stopped by %s after %d iterations: true relative residual %.3g (tol %.3g)"
                      % (info["status"], info["iterations"], info["true_residual"], float(tol)), RuntimeWarning, stacklevel=2)
    return V, info


def _potential_of_graph(ref_nodes, pos, ptr, nbr, r, tol, max_iter, device):
    """what calc_diff_potential does with the graph it read: r by node name -> the vector, the solve, the dict"""
    n, ptr, nbr = _check_graph(ptr, nbr)
    _check_params(tol, max_iter)
    rvec = None
    if r is not None:
        rvec = np.ones(n, dtype=np.float64)                    # a node of the file that is not in refNodes keeps 1
        for x in ref_nodes:
            if x not in r:
                print('ERROR: %s node is missing in r')          # the reference's line, its unfilled %s included
                return {}
            rvec[pos[x]] = r[x]
        if not np.isfinite(rvec).all():
            raise ValueError("ERROR: r holds a value that is not finite")
    V, _ = diff_potential_csr(ptr, nbr, rvec, tol, max_iter, device)
    return {x: float(V[pos[x]]) for x in ref_nodes}


def calc_diff_potential(mapping_h5_fn, ref_name, r=None, tol=1e-10, max_iter=10000, device=0):
    """Graph.calc_diff_potential (nabo/_graph.py:918-954) from the mapping file: {reference node: V}, V = pinv(I - A/D) r
    on the unweighted reference graph, in the file's node order (`refNodes`; the reference's own dict follows networkx's
    view of refG, the values per node are the same).  Smaller values are less differentiated cells.

    r: {reference node: rate}, None = all ones.  As in the reference, a node missing from r prints the reference's line
    and returns {} (a quirk, kept); a value that is not finite raises ValueError.  A reference node without any edge
    raises ValueError before the device is touched (the reference divides by zero there and pinv raises).

    What differs from the reference: no dense matrix.  The same vector solves one sparse symmetric system per connected
    component, taken by conjugate gradients to `tol` (relative residual) in at most `max_iter` iterations; a run that
    does not converge returns its iterate and issues a RuntimeWarning with the true residual."""
    ref_nodes, pos, _, ptr, nbr, _ = read_ref_graph(mapping_h5_fn, ref_name)
    return _potential_of_graph(ref_nodes, pos, ptr, nbr, r, tol, max_iter, device)
