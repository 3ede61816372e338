"""What the graph steps (_layout, _umap, _community, _potential, _paths) share on the Python side: the checks of a CSR
argument, the reference graph of a mapping file as a CSR by node id, and the owner of a handle of the C library.
"""
import numpy as np

from . import _lib


def _f64(a, name, n=None):
    try:
        a = np.ascontiguousarray(a, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("ERROR: %s must be numeric" % name)
    if a.ndim != 1 or (n is not None and a.shape[0] != n):
        raise ValueError("ERROR: %s must be 1-D%s" % (name, "" if n is None else " with %d entries" % n))
    if not np.isfinite(a).all():
        raise ValueError("ERROR: %s holds a value that is not finite" % name)
    return a


def check_csr(ptr, nbr, w=None):
    """(n, ptr, nbr) as int64, and w as float64 if given: a graph of n >= 1 nodes, ptr from 0 to len(nbr), nbr in [0, n)"""
    try:
        ptr, nbr = np.ascontiguousarray(ptr, dtype=np.int64), np.ascontiguousarray(nbr, dtype=np.int64)
    except (TypeError, ValueError, OverflowError):
        raise ValueError("ERROR: ptr and nbr must be integers")
    if ptr.ndim != 1 or nbr.ndim != 1:
        raise ValueError("ERROR: ptr and nbr must be 1-D")
    if w is not None:
        w = _f64(w, "w", nbr.shape[0])
    n = ptr.shape[0] - 1
    if n < 1:
        raise ValueError("ERROR: ptr needs n_nodes + 1 entries and the graph at least one node")
    if ptr[0] != 0 or (np.diff(ptr) < 0).any() or int(ptr[-1]) != nbr.shape[0]:
        raise ValueError("ERROR: ptr must start at 0, be monotone and end at len(nbr) = %d" % nbr.shape[0])
    if nbr.size and (nbr.min() < 0 or nbr.max() >= n):
        raise ValueError("ERROR: nbr holds an entry that is not a node in [0, %d)" % n)
    return (n, ptr, nbr) if w is None else (n, ptr, nbr, w)


def csr_by_node_id(rows, pos, n_ref, ptr, nbr, w=None):
    """The rows of the file (node names `rows`, pos: name -> node id = position in ref_cells) as a CSR by node id, the
    arcs of a node in the file's order (either arc direction will do): (ptr [n_ref + 1], nbr, w or None)"""
    src = np.repeat(np.array([pos[r] for r in rows], dtype=np.int64), np.diff(ptr))
    order = np.argsort(src, kind="stable")
    cptr = np.zeros(n_ref + 1, dtype=np.int64)
    np.cumsum(np.bincount(src, minlength=n_ref), out=cptr[1:])
    return cptr, nbr[order], None if w is None else w[order]


def open_ref(h5, ref_name):
    """(node names by node id, name -> node id, the reference's uid) of an open mapping file"""
    if h5["name_stash/ref_name"][0].decode("UTF-8") != ref_name:
        raise KeyError("ERROR: The reference is named %s in the mapping file and not %s. Please verify that you are "
                       "trying to load right reference." % (h5["name_stash/ref_name"][0].decode("UTF-8"), ref_name))
    cells = [x.decode("UTF-8") for x in h5["ref_cells/ref_cells"][:]]
    names = [c + "_" + ref_name for c in cells]
    return names, {n: i for i, n in enumerate(names)}, h5["name_stash/ref_name"][1].decode("UTF-8")


def read_ref_graph(mapping_h5_fn, ref_name):
    """(refNodes, node -> id, n_ref, a CSR by node id with the file's weights): the reference graph of a mapping file"""
    import h5py
    from ._mapping import read_graph_csr
    with h5py.File(mapping_h5_fn, "r") as h5:
        names, pos, ref_uid = open_ref(h5, ref_name)
        rows, ptr, nbr, w = read_graph_csr(h5[ref_uid + "_graph"], pos)
    return (list(rows), pos, len(names)) + csr_by_node_id(rows, pos, len(names), ptr, nbr, w)


class Handle:
    """Owns one handle of the C library, `_h`, made by the subclass's __init__ and freed by the function `_destroy`
    names; a context manager, and freed with the object at the latest."""
    _destroy = None
    _h = None

    def close(self):
        if self._h is not None:
            getattr(_lib.lib(), self._destroy)(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
