"""UMAP embedding of cells on the GPU: exact k-NN, fuzzy graph, synchronous epochs.

Array / HDF5 restatement of `nabo.make_umap` (nabo/_umap.py:7-39).  The reference hands the PCA coordinates to
`umap.UMAP`; here `nabo_umap_*` (include/nabo_umap.h, nabo_amd/csrc/umap.hip) takes the k-NN lists from the resident
index, builds umap's fuzzy graph on the device and runs the optimisation as synchronous epochs, so the same call gives
the same bits every time.  include/nabo_umap.h holds the definition; umap-learn's own floating-point results and its
random stream are not pinned.  What stays on the host is small: the fit of the curve's a and b and the
start positions.

`umap_transform` / `make_target_umap` place a SECOND set of cells, the targets, in a fitted embedding that does not move
(`nabo_umap_transform_*`, include/nabo_umap_transform.h, nabo_amd/csrc/umap_transform.hip): what
umap-learn users call `UMAP.transform`.  A target's result depends on its row, its global row number, the reference and
the parameters only, so any split into batches gives the same bits.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._graphio import Handle
from ._lib import EUCLIDEAN

KERNEL_MS = ("graph", "knn", "epoch", "run")


def geometry():
    """lanes that share one node's row in the epoch kernel (the order of a node's sum); needs no device"""
    g = C.c_int32()
    _lib.check(_lib.lib().nabo_umap_geometry(C.byref(g)))
    return int(g.value)


def default_n_epochs(n):
    """umap-learn's choice: 500 for up to 10000 cells, 200 above"""
    return 500 if int(n) <= 10000 else 200


def _number(v, name, positive=False):
    try:
        v = float(v)
    except (TypeError, ValueError):
        raise ValueError("ERROR: %s must be a number" % name)
    if not np.isfinite(v) or (positive and not v > 0):
        raise ValueError("ERROR: %s must be finite%s" % (name, " and positive" if positive else ""))
    return v


def _count(v, name, least):
    try:
        ok = int(v) == v
    except (TypeError, ValueError):
        ok = False
    if not ok or int(v) < least:
        raise ValueError("ERROR: %s must be a whole number, at least %d" % (name, least))
    return int(v)


def curve(spread, min_dist):
    """umap's target curve: 300 points x on [0, 3 spread], 1 below min_dist and exp(-(x - min_dist) / spread) above"""
    x = np.linspace(0.0, 3.0 * spread, 300)
    y = np.ones(300)
    far = x >= min_dist
    y[far] = np.exp(-(x[far] - min_dist) / spread)
    return x, y


def find_ab_params(spread=1.0, min_dist=0.1):
    """(a, b) of 1 / (1 + a x^(2b)) fitted to `curve(spread, min_dist)` by least squares, as umap's find_ab_params does
    with scipy's curve_fit -- here a Levenberg-Marquardt in numpy from a = b = 1, so that the GPU machine needs no
    scipy.  Both are minima of the same smooth problem; tests/test_umap_cpu.py compares the two fitted curves."""
    spread, min_dist = _number(spread, "spread", True), _number(min_dist, "min_dist")
    if min_dist < 0 or min_dist >= 3.0 * spread:
        raise ValueError("ERROR: min_dist must be in [0, 3 * spread)")
    x, y = curve(spread, min_dist)
    xs, ys = x[1:], y[1:]                       # x = 0 fits exactly whatever a and b are
    lx = np.log(xs)

    def resid(p):
        return 1.0 / (1.0 + p[0] * xs ** (2.0 * p[1])) - ys

    p = np.array([1.0, 1.0])
    r = resid(p)
    cost, lam = float(r @ r), 1e-3
    for _ in range(200):
        u = xs ** (2.0 * p[1])
        f = 1.0 / (1.0 + p[0] * u)
        J = np.stack([-f * f * u, -f * f * p[0] * u * 2.0 * lx], axis=1)
        A, g = J.T @ J, J.T @ r
        moved = False
        for _ in range(40):
            step = np.linalg.solve(A + lam * np.diag(np.diag(A)), -g)
            q = p + step
            if q[0] > 0 and q[1] > 0:
                rq = resid(q)
                cq = float(rq @ rq)
                if cq <= cost:
                    moved = True
                    break
            lam *= 10.0
        if not moved:
            break
        small = abs(cost - cq) <= 1e-16 * max(cost, 1e-300) and np.max(np.abs(step)) <= 1e-12 * np.max(np.abs(p))
        p, r, cost, lam = q, rq, cq, max(lam / 10.0, 1e-12)
        if small:
            break
    return float(p[0]), float(p[1])


def scale_start(y):
    """umap's rescaling of a start, in float64: each dimension to [0, 10]; a constant column to 0"""
    y = np.array(y, dtype=np.float64)
    mn, mx = y.min(axis=0), y.max(axis=0)
    span = mx - mn
    out = np.zeros_like(y)
    ok = span > 0
    out[:, ok] = (10.0 * (y[:, ok] - mn[ok])) / span[ok]
    return out


def start_positions(init, X, n, dims, seed):
    """part E of include/nabo_umap.h: "pca" = the first `dims` columns of X (the inputs are PCA coordinates, so this is
    umap's spectral start without an eigen-solver), "random" = default_rng(seed).uniform(-10, 10), or an [n, dims]
    array; each brought to [0, 10] per dimension"""
    if isinstance(init, str):
        if init == "pca":
            if X is None or X.shape[1] < dims:
                raise ValueError("ERROR: init='pca' needs at least %d components" % dims)
            y = X[:, :dims]
        elif init == "random":
            y = np.random.default_rng(seed).uniform(-10.0, 10.0, size=(n, dims))
        else:
            raise ValueError("ERROR: init must be 'pca', 'random' or an [n, dims] array")
    else:
        try:
            y = np.asarray(init, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError("ERROR: init must be 'pca', 'random' or an [n, dims] array")
        if y.shape != (n, dims):
            raise ValueError("ERROR: init must be [n, dims] = [%d, %d]" % (n, dims))
    if not np.isfinite(y).all():
        raise ValueError("ERROR: the start holds a value that is not finite")
    return scale_start(y)


def _check_lists(idx, dist):
    try:
        idx = np.ascontiguousarray(idx, dtype=np.int64)
        dist = np.ascontiguousarray(dist, dtype=np.float64)
    except (TypeError, ValueError, OverflowError):
        raise ValueError("ERROR: idx must be integers and dist numbers")
    if idx.ndim != 2 or idx.shape != dist.shape:
        raise ValueError("ERROR: idx and dist must both be [n, k]")
    n, k = idx.shape
    if k < 2 or k > _lib.MAX_K or k >= n:
        raise ValueError("ERROR: k=%d must be in [2, %d] and below n=%d" % (k, _lib.MAX_K, n))
    if idx.min() < 0 or idx.max() >= n:
        raise ValueError("ERROR: idx holds an entry that is not a cell in [0, %d)" % n)
    if not np.isfinite(dist).all() or (dist < 0).any() or (np.diff(dist, axis=1) < 0).any():
        raise ValueError("ERROR: dist must be finite, not negative and ascending along every row")
    s = np.sort(idx, axis=1)
    if (s[:, 1:] == s[:, :-1]).any():
        raise ValueError("ERROR: a row of idx names a cell twice")
    return idx, dist


class Umap(Handle):
    """An embedding resident on one device (nabo_umap_create): the handle the tests and tools/bench_umap.py step
    through; `umap_fit` is the one-call form."""
    _destroy = "nabo_umap_destroy"

    def __init__(self, n, dims=2, device=0, n_epochs=None, negative_sample_rate=5, repulsion_strength=1.0, a=None, b=None,
                 seed=0):
        self.n, self.dims = _count(n, "n", 3), _count(dims, "dims", 2)
        if self.dims > 3:
            raise ValueError("ERROR: dims must be 2 or 3")
        p = self._params(n_epochs, negative_sample_rate, repulsion_strength, a, b, seed)
        h = C.c_void_p()
        _lib.check(_lib.lib().nabo_umap_create(C.byref(h), int(device), self.n, self.dims))
        self._h = h
        self._apply(p)

    def _params(self, n_epochs, negative_sample_rate, repulsion_strength, a, b, seed):
        if (a is None) != (b is None):
            raise ValueError("ERROR: give both a and b or neither")
        if a is None:
            a, b = find_ab_params(1.0, 0.1)
        return dict(n_epochs=default_n_epochs(self.n) if n_epochs is None else _count(n_epochs, "n_epochs", 1),
                    negative_sample_rate=_count(negative_sample_rate, "negative_sample_rate", 1),
                    repulsion_strength=_number(repulsion_strength, "repulsion_strength"), a=_number(a, "a", True),
                    b=_number(b, "b", True), seed=_count(seed, "seed", 0) & (2 ** 64 - 1))

    def _apply(self, p):
        _lib.check(_lib.lib().nabo_umap_set_params(self._h, p["n_epochs"], p["negative_sample_rate"], p["repulsion_strength"],
                                                   p["a"], p["b"], p["seed"]))
        self.params = p

    def set_params(self, **kw):
        """any of n_epochs, negative_sample_rate, repulsion_strength, a and b, seed; rewinds the schedule, and a graph built
        for another n_epochs is dropped"""
        unknown = sorted(set(kw) - set(self.params))
        if unknown:
            raise ValueError("ERROR: unknown parameter(s): %s" % ", ".join(unknown))
        p = dict(self.params, **kw)
        self._apply(self._params(p["n_epochs"], p["negative_sample_rate"], p["repulsion_strength"], p["a"], p["b"], p["seed"]))
        return self

    def set_knn(self, idx, dist):
        idx, dist = _check_lists(idx, dist)
        if idx.shape[0] != self.n:
            raise ValueError("ERROR: the lists must have n = %d rows" % self.n)
        _lib.check(_lib.lib().nabo_umap_set_knn(self._h, idx.ctypes.data, dist.ctypes.data, idx.shape[1]))
        return self

    def fit_knn(self, X, n_neighbors, metric=EUCLIDEAN, dist_factor=0.25):
        """the lists from the resident k-NN index, X against X: they never visit the host"""
        X = _cells(X, self.n)
        k = _count(n_neighbors, "n_neighbors", 2)
        if k > _lib.MAX_K or k >= self.n:
            raise ValueError("ERROR: n_neighbors=%d must be in [2, %d] and below n=%d" % (k, _lib.MAX_K, self.n))
        _lib.check(_lib.lib().nabo_umap_fit_knn(self._h, X.ctypes.data, X.shape[1], k, int(metric), float(dist_factor)))
        return self

    def set_graph(self, ptr, nbr, w):
        """a finished CSR (as `graph` returns it) in place of the lists: nothing is pruned or sorted"""
        try:
            ptr, nbr = np.ascontiguousarray(ptr, dtype=np.int64), np.ascontiguousarray(nbr, dtype=np.int64)
            w = np.ascontiguousarray(w, dtype=np.float64)
        except (TypeError, ValueError, OverflowError):
            raise ValueError("ERROR: ptr and nbr must be integers and w numbers")
        if ptr.shape != (self.n + 1,) or nbr.ndim != 1 or w.shape != nbr.shape or int(ptr[-1]) != nbr.shape[0]:
            raise ValueError("ERROR: ptr must be [n + 1], nbr and w [ptr[n]]")
        _lib.check(_lib.lib().nabo_umap_set_graph(self._h, ptr.ctypes.data, nbr.ctypes.data, w.ctypes.data))
        return self

    def graph(self):
        """(rho, sigma, ptr, nbr, w): the smooth distances and the pruned symmetric CSR, rows in ascending neighbour"""
        E, wmax = C.c_int64(), C.c_double()
        _lib.check(_lib.lib().nabo_umap_graph_size(self._h, C.byref(E), C.byref(wmax)))
        rho, sigma = np.empty(self.n), np.empty(self.n)
        ptr, nbr, w = np.empty(self.n + 1, dtype=np.int64), np.empty(E.value, dtype=np.int64), np.empty(E.value)
        _lib.check(_lib.lib().nabo_umap_get_graph(self._h, rho.ctypes.data, sigma.ctypes.data, ptr.ctypes.data, nbr.ctypes.data,
                                                  w.ctypes.data))
        return rho, sigma, ptr, nbr, w

    def set_embedding(self, y):
        try:
            y = np.ascontiguousarray(y, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError("ERROR: y must be numeric")
        if y.shape != (self.n, self.dims):
            raise ValueError("ERROR: y must be [n, dims] = [%d, %d]" % (self.n, self.dims))
        _lib.check(_lib.lib().nabo_umap_set_embedding(self._h, y.ctypes.data))
        return self

    def get_embedding(self):
        y = np.empty((self.n, self.dims), dtype=np.float64)
        _lib.check(_lib.lib().nabo_umap_get_embedding(self._h, y.ctypes.data))
        return y

    def run(self, n_run=None):
        """the next n_run epochs (default: all that are left), never past n_epochs; returns how many ran"""
        done = C.c_int64()
        _lib.check(_lib.lib().nabo_umap_run(self._h, self.params["n_epochs"] if n_run is None else int(n_run), C.byref(done)))
        return int(done.value)

    def rewind(self):
        _lib.check(_lib.lib().nabo_umap_rewind(self._h))
        return self

    def last_epoch_counts(self):
        """{"n_attr", "n_neg": int32 [n], "idx_sum": uint64 [n]} of the last epoch run"""
        a, b, s = np.empty(self.n, dtype=np.int32), np.empty(self.n, dtype=np.int32), np.empty(self.n, dtype=np.uint64)
        _lib.check(_lib.lib().nabo_umap_last_epoch_counts(self._h, a.ctypes.data, b.ctypes.data, s.ctypes.data))
        return {"n_attr": a, "n_neg": b, "idx_sum": s}

    def last_ms(self):
        """{"graph", "knn", "epoch" (mean per epoch over the last `n_timed`), "run": device ms, "n_timed"}"""
        ms = (C.c_double * 4)()
        nt = C.c_int64()
        _lib.check(_lib.lib().nabo_umap_last_ms(self._h, ms, C.byref(nt)))
        out = dict(zip(KERNEL_MS, ms[:4]))
        out["n_timed"] = int(nt.value)
        return out


def _cells(X, n=None):
    try:
        X = np.ascontiguousarray(X, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("ERROR: X must be numeric")
    if X.ndim != 2 or X.shape[1] < 1 or (n is not None and X.shape[0] != n):
        raise ValueError("ERROR: X must be [n_cells, n_comps]%s" % ("" if n is None else " with %d rows" % n))
    if not np.isfinite(X).all():
        raise ValueError("ERROR: X holds a value that is not finite")
    return X


def umap_fuzzy_graph(idx, dist, n_epochs=None, device=0):
    """(rho, sigma, ptr, nbr, w) of the k-NN lists idx, dist [n, k] (each cell's k nearest, itself included, ascending):
    umap's smooth distances and its fuzzy union graph as a symmetric CSR, arcs below max(w) / n_epochs pruned"""
    idx, dist = _check_lists(idx, dist)
    with Umap(idx.shape[0], 2, device, n_epochs=n_epochs, a=1.0, b=1.0) as U:
        return U.set_knn(idx, dist).graph()


def umap_fit(X, n_neighbors=15, dims=2, n_epochs=None, spread=1.0, min_dist=0.1, repulsion_strength=1.0,
             negative_sample_rate=5, seed=0, init="pca", metric=EUCLIDEAN, dist_factor=0.25, a=None, b=None, device=0):
    """The UMAP embedding of the cells X [n, n_comps], float64 [n, dims]: exact k-NN of X against itself on the device,
    the fuzzy graph, then n_epochs synchronous epochs (include/nabo_umap.h) from the start `init` ("pca": the first
    `dims` columns of X; "random"; or an [n, dims] array).  a and b default to `find_ab_params(spread, min_dist)`;
    n_epochs=None means 500 for up to 10000 cells and 200 above.  The same call returns the same bits."""
    X = _cells(X)
    n = X.shape[0]
    dims = _count(dims, "dims", 2)
    if dims > 3:
        raise ValueError("ERROR: dims must be 2 or 3")
    if n < 3:
        raise ValueError("ERROR: at least 3 cells are needed")
    k = _count(n_neighbors, "n_neighbors", 2)
    if k > _lib.MAX_K or k >= n:
        raise ValueError("ERROR: n_neighbors=%d must be in [2, %d] and below n=%d" % (k, _lib.MAX_K, n))
    if a is None and b is None:
        a, b = find_ab_params(spread, min_dist)
    seed = _count(seed, "seed", 0)
    y0 = start_positions(init, X, n, dims, seed)
    with Umap(n, dims, device, n_epochs=n_epochs, negative_sample_rate=negative_sample_rate,
              repulsion_strength=repulsion_strength, a=a, b=b, seed=seed) as U:
        U.fit_knn(X, n_neighbors, metric, dist_factor)
        U.set_embedding(y0)
        U.run()
        return U.get_embedding()


def _read_cells(pca_h5, data_group, use_comps):
    from ._mapping import _read_group_matrix
    return _read_group_matrix(pca_h5, data_group, None, int(use_comps))


def make_umap(pca_h5, use_comps, umap_dims, n_neighbors, spread, repulsion_strength, min_dist, n_epochs, data_group="data",
              index_suffix="", verbose=True, *, seed=0, init="pca", negative_sample_rate=5, device=0):
    """nabo.make_umap (nabo/_umap.py:7-39): the UMAP embedding of the cells of a PCA file, as the reference's DataFrame:
    one row per cell, named cell + index_suffix, columns Dim1 .. Dim<umap_dims>.  Reads the per-cell groups
    `transform_pca` writes and the dense layout of `write_dense_pca`, cells in the file's name order.

    What differs from the reference: the vectors are read from `data_group`, where the reference lists the cells of
    `data_group` but reads their vectors from the hard-wired group 'data' (line 31: the two agree only for the default);
    the neighbours are exact; the epochs are synchronous and seeded (`seed`), so the same call gives the same frame, bit
    for bit; the start is the first `umap_dims` PCA components (`init`), not a spectral layout; n_epochs=None means 500
    for up to 10000 cells, else 200.  pandas and h5py are imported when the function is called."""
    import pandas as pd
    cells, Z = _read_cells(pca_h5, data_group, use_comps)
    Y = umap_fit(Z, n_neighbors, umap_dims, n_epochs, spread, min_dist, repulsion_strength, negative_sample_rate, seed, init,
                 device=device)
    if verbose:
        print("UMAP of %d cells in %d dimensions: %d neighbours, %d epochs"
              % (len(cells), int(umap_dims), int(n_neighbors), default_n_epochs(len(cells)) if n_epochs is None else int(n_epochs)))
    return pd.DataFrame(Y, index=[x + index_suffix for x in cells], columns=["Dim" + str(x) for x in range(1, int(umap_dims) + 1)])


# ---------------------------------------------------------------------------------------------------------------------
# transform: target cells placed in a fitted reference embedding

TRANSFORM_MS = ("graph", "knn", "run")


def transform_geometry():
    """lanes that share one target's list in the optimise kernel (the order of a target's sum); needs no device"""
    g = C.c_int32()
    _lib.check(_lib.lib().nabo_umap_transform_geometry(C.byref(g)))
    return int(g.value)


def default_transform_epochs(m):
    """umap-learn's choice for transform: 100 for up to 10000 targets, 30 above"""
    return 100 if int(m) <= 10000 else 30


def _check_target_lists(idx, val, n_ref, memberships=False):
    """idx, val [m, k] of a batch: val the ascending distances, or memberships in [0, 1]"""
    try:
        idx = np.ascontiguousarray(idx, dtype=np.int64)
        val = np.ascontiguousarray(val, dtype=np.float64)
    except (TypeError, ValueError, OverflowError):
        raise ValueError("ERROR: idx must be integers and %s numbers" % ("memb" if memberships else "dist"))
    if idx.ndim != 2 or idx.shape != val.shape or idx.shape[0] < 1:
        raise ValueError("ERROR: idx and %s must both be [m, k], m at least 1" % ("memb" if memberships else "dist"))
    k = idx.shape[1]
    if k < 2 or k > _lib.MAX_K or k > n_ref:
        raise ValueError("ERROR: k=%d must be in [2, %d] and not above n_ref=%d" % (k, _lib.MAX_K, n_ref))
    if idx.min() < 0 or idx.max() >= n_ref:
        raise ValueError("ERROR: idx holds an entry that is not a reference cell in [0, %d)" % n_ref)
    if memberships:
        if not np.isfinite(val).all() or (val < 0).any() or (val > 1).any():
            raise ValueError("ERROR: memb must be finite and in [0, 1]")
    elif not np.isfinite(val).all() or (val < 0).any() or (np.diff(val, axis=1) < 0).any():
        raise ValueError("ERROR: dist must be finite, not negative and ascending along every row")
    return idx, val


def _neighbours(n_neighbors, n_ref):
    k = _count(n_neighbors, "n_neighbors", 2)
    if k > _lib.MAX_K or k > n_ref:
        raise ValueError("ERROR: n_neighbors=%d must be in [2, %d] and not above n_ref=%d" % (k, _lib.MAX_K, n_ref))
    return k


class UmapTransform(Handle):
    """A fitted reference embedding resident on one device (nabo_umap_transform_create) and one batch of target cells
    at a time: the handle the tests and tools/bench_umap_transform.py step through; `umap_transform` is the one-call
    form."""
    _destroy = "nabo_umap_transform_destroy"

    def __init__(self, n_ref, dims=2, device=0, n_epochs=None, negative_sample_rate=5, repulsion_strength=1.0, a=None, b=None,
                 seed=0):
        self.n_ref, self.dims = _count(n_ref, "n_ref", 2), _count(dims, "dims", 2)
        if self.dims > 3:
            raise ValueError("ERROR: dims must be 2 or 3")
        self.m = self.k = self.g = 0
        p = self._params(n_epochs, negative_sample_rate, repulsion_strength, a, b, seed)
        h = C.c_void_p()
        _lib.check(_lib.lib().nabo_umap_transform_create(C.byref(h), int(device), self.n_ref, self.dims))
        self._h = h
        self._apply(p)

    def _params(self, n_epochs, negative_sample_rate, repulsion_strength, a, b, seed):
        if (a is None) != (b is None):
            raise ValueError("ERROR: give both a and b or neither")
        if a is None:
            a, b = find_ab_params(1.0, 0.1)
        return dict(n_epochs=100 if n_epochs is None else _count(n_epochs, "n_epochs", 1),
                    negative_sample_rate=_count(negative_sample_rate, "negative_sample_rate", 1),
                    repulsion_strength=_number(repulsion_strength, "repulsion_strength"), a=_number(a, "a", True),
                    b=_number(b, "b", True), seed=_count(seed, "seed", 0) & (2 ** 64 - 1))

    def _apply(self, p):
        _lib.check(_lib.lib().nabo_umap_transform_set_params(self._h, p["n_epochs"], p["negative_sample_rate"],
                                                             p["repulsion_strength"], p["a"], p["b"], p["seed"]))
        self.params = p

    def set_params(self, **kw):
        """any of n_epochs, negative_sample_rate, repulsion_strength, a and b, seed; rewinds a loaded batch's schedule"""
        unknown = sorted(set(kw) - set(self.params))
        if unknown:
            raise ValueError("ERROR: unknown parameter(s): %s" % ", ".join(unknown))
        p = dict(self.params, **kw)
        self._apply(self._params(p["n_epochs"], p["negative_sample_rate"], p["repulsion_strength"], p["a"], p["b"], p["seed"]))
        return self

    def set_embedding(self, Y):
        """the fitted reference positions [n_ref, dims]"""
        _lib.check(_lib.lib().nabo_umap_transform_set_embedding(self._h, _positions(Y, self.n_ref, self.dims, "Y").ctypes.data))
        return self

    def set_cells(self, X, metric=EUCLIDEAN, dist_factor=0.25):
        """the reference cells [n_ref, n_comps] as a resident k-NN index, kept for every batch that follows"""
        X = _cells(X, self.n_ref)
        _lib.check(_lib.lib().nabo_umap_transform_set_cells(self._h, X.ctypes.data, X.shape[1], int(metric), float(dist_factor)))
        self.g = X.shape[1]
        return self

    def _first_row(self, first_row):
        return _count(first_row, "first_row", 0)

    def query(self, Z, n_neighbors, first_row=0):
        """one batch from its cells Z [m, n_comps]: the lists come from the resident index and never visit the host"""
        if not self.g:
            raise ValueError("ERROR: no reference cells: call set_cells first")
        Z = _cells(Z)
        if Z.shape[0] < 1 or Z.shape[1] != self.g:
            raise ValueError("ERROR: Z must be [m, %d] with at least one row" % self.g)
        k, first_row = _neighbours(n_neighbors, self.n_ref), self._first_row(first_row)
        _lib.check(_lib.lib().nabo_umap_transform_query(self._h, Z.shape[0], first_row, Z.ctypes.data, k))
        self.m, self.k = Z.shape[0], k
        return self

    def set_knn(self, idx, dist, first_row=0):
        idx, dist = _check_target_lists(idx, dist, self.n_ref)
        first_row = self._first_row(first_row)
        _lib.check(_lib.lib().nabo_umap_transform_set_knn(self._h, idx.shape[0], first_row, idx.ctypes.data, dist.ctypes.data, idx.shape[1]))
        self.m, self.k = idx.shape
        return self

    def set_graph(self, idx, memb, first_row=0):
        """memberships [m, k] in [0, 1] in place of the smooth distances (for the tests)"""
        idx, memb = _check_target_lists(idx, memb, self.n_ref, memberships=True)
        first_row = self._first_row(first_row)
        _lib.check(_lib.lib().nabo_umap_transform_set_graph(self._h, idx.shape[0], first_row, idx.ctypes.data, memb.ctypes.data, idx.shape[1]))
        self.m, self.k = idx.shape
        return self

    def _batch(self):
        if not self.m:
            raise ValueError("ERROR: no batch: call query, set_knn or set_graph first")

    def graph(self):
        """(sigma [m], memb [m, k], y0 [m, dims]) of the loaded batch"""
        self._batch()
        sigma, memb, y0 = np.empty(self.m), np.empty((self.m, self.k)), np.empty((self.m, self.dims))
        _lib.check(_lib.lib().nabo_umap_transform_get_graph(self._h, sigma.ctypes.data, memb.ctypes.data, y0.ctypes.data))
        return sigma, memb, y0

    def set_positions(self, y):
        self._batch()
        _lib.check(_lib.lib().nabo_umap_transform_set_positions(self._h, _positions(y, self.m, self.dims, "y").ctypes.data))
        return self

    def get_positions(self):
        self._batch()
        y = np.empty((self.m, self.dims), dtype=np.float64)
        _lib.check(_lib.lib().nabo_umap_transform_get_positions(self._h, y.ctypes.data))
        return y

    def run(self, n_run=None):
        """the next n_run epochs (default: all that are left) in one launch, never past n_epochs; returns how many ran"""
        self._batch()
        done = C.c_int64()
        _lib.check(_lib.lib().nabo_umap_transform_run(self._h, self.params["n_epochs"] if n_run is None else int(n_run), C.byref(done)))
        return int(done.value)

    def rewind(self):
        self._batch()
        _lib.check(_lib.lib().nabo_umap_transform_rewind(self._h))
        return self

    def last_run_counts(self):
        """{"n_attr", "n_neg": int64 [m], "idx_sum": uint64 [m]} over the epochs of the last run"""
        self._batch()
        a, b, s = np.empty(self.m, dtype=np.int64), np.empty(self.m, dtype=np.int64), np.empty(self.m, dtype=np.uint64)
        _lib.check(_lib.lib().nabo_umap_transform_last_run_counts(self._h, a.ctypes.data, b.ctypes.data, s.ctypes.data))
        return {"n_attr": a, "n_neg": b, "idx_sum": s}

    def last_ms(self):
        """{"graph", "knn", "run"}: device ms of the last batch's graph build, its k-NN and the last run"""
        ms = (C.c_double * 3)()
        _lib.check(_lib.lib().nabo_umap_transform_last_ms(self._h, ms))
        return dict(zip(TRANSFORM_MS, ms[:3]))


def _positions(y, n, dims, name):
    try:
        y = np.ascontiguousarray(y, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("ERROR: %s must be numeric" % name)
    if y.shape != (n, dims):
        raise ValueError("ERROR: %s must be [%d, %d]" % (name, n, dims))
    if not np.isfinite(y).all():
        raise ValueError("ERROR: %s holds a value that is not finite" % name)
    return y


def umap_transform(Z, X_ref, ref_embedding, n_neighbors=15, n_epochs=None, spread=1.0, min_dist=0.1, repulsion_strength=1.0,
                   negative_sample_rate=5, seed=0, metric=EUCLIDEAN, dist_factor=0.25, a=None, b=None, device=0, batch=None):
    """The positions, float64 [m, dims], of the target cells Z [m, n_comps] in the fitted embedding `ref_embedding`
    [n_ref, dims] of the reference cells X_ref [n_ref, n_comps]; the reference does not move
    (include/nabo_umap_transform.h).  a and b default to `find_ab_params(spread, min_dist)`; n_epochs=None means umap's
    100 for up to 10000 targets and 30 above, a given n_epochs is used as given.  The targets go through in batches of
    `batch` rows (None: all at once) with their global row numbers: every split returns the same bits."""
    Z, X_ref = _cells(Z), _cells(X_ref)
    m, n_ref = Z.shape[0], X_ref.shape[0]
    if m < 1 or n_ref < 2:
        raise ValueError("ERROR: at least 1 target and 2 reference cells are needed")
    if Z.shape[1] != X_ref.shape[1]:
        raise ValueError("ERROR: Z and X_ref must have the same number of components")
    try:
        Y = np.ascontiguousarray(ref_embedding, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("ERROR: ref_embedding must be numeric")
    if Y.ndim != 2 or Y.shape[0] != n_ref or Y.shape[1] not in (2, 3):
        raise ValueError("ERROR: ref_embedding must be [n_ref, 2] or [n_ref, 3] with n_ref = %d" % n_ref)
    Y = _positions(Y, n_ref, Y.shape[1], "ref_embedding")
    k = _neighbours(n_neighbors, n_ref)
    if a is None and b is None:
        a, b = find_ab_params(spread, min_dist)
    seed = _count(seed, "seed", 0)
    n_epochs = default_transform_epochs(m) if n_epochs is None else _count(n_epochs, "n_epochs", 1)
    batch = m if batch is None else _count(batch, "batch", 1)
    out = np.empty((m, Y.shape[1]), dtype=np.float64)
    with UmapTransform(n_ref, Y.shape[1], device, n_epochs=n_epochs, negative_sample_rate=negative_sample_rate,
                       repulsion_strength=repulsion_strength, a=a, b=b, seed=seed) as T:
        T.set_embedding(Y)
        T.set_cells(X_ref, metric, dist_factor)
        for r0 in range(0, m, batch):
            T.query(Z[r0:r0 + batch], k, first_row=r0)
            T.run()
            out[r0:r0 + batch] = T.get_positions()
    return out


def make_target_umap(ref_pca_h5, target_pca_h5, ref_umap, use_comps, n_neighbors, spread=1.0, repulsion_strength=1.0, min_dist=0.1,
                     n_epochs=None, data_group="data", index_suffix="", verbose=True, *, ref_data_group="data", seed=0,
                     negative_sample_rate=5, device=0, batch=None):
    """The target cells of a PCA file placed in the reference's UMAP, as a frame of the reference frame's shape: one row
    per target cell, named cell + index_suffix, with the columns of `ref_umap` -- the frame `make_umap` returned for
    `ref_pca_h5`, whose row count is checked against that file (its rows are the file's cells in name order).  The
    reference's vectors are read from `ref_data_group` of `ref_pca_h5`, the targets' from `data_group` of
    `target_pca_h5`, the first `use_comps` components of each.  pandas and h5py are imported when the function is
    called."""
    import pandas as pd
    try:
        Y = np.ascontiguousarray(ref_umap.values, dtype=np.float64)
        columns = list(ref_umap.columns)
    except (AttributeError, TypeError, ValueError):
        raise ValueError("ERROR: ref_umap must be the frame make_umap returned")
    ref_cells, X = _read_cells(ref_pca_h5, ref_data_group, use_comps)
    if Y.ndim != 2 or Y.shape[0] != len(ref_cells):
        raise ValueError("ERROR: ref_umap has %d rows, the reference file %d cells" % (Y.shape[0] if Y.ndim else 0, len(ref_cells)))
    cells, Z = _read_cells(target_pca_h5, data_group, use_comps)
    P = umap_transform(Z, X, Y, n_neighbors, n_epochs, spread, min_dist, repulsion_strength, negative_sample_rate, seed,
                       device=device, batch=batch)
    if verbose:
        print("UMAP transform of %d cells onto %d reference cells: %d neighbours, %d epochs"
              % (len(cells), len(ref_cells), int(n_neighbors), default_transform_epochs(len(cells)) if n_epochs is None else int(n_epochs)))
    return pd.DataFrame(P, index=[x + index_suffix for x in cells], columns=columns)
