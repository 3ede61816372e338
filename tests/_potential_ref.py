"""numpy restatement of include/nabo_potential.h, the yardstick of the potential tests: the simple graph, components, the
projected right-hand side, the preconditioned conjugate gradients one iteration at a time, the minimum-norm step, and
the dense route (numpy.linalg.pinv of I - A/D, the smallest non-zero eigenvalue of K) it is held against.  Written from
the header's definition; nothing here is shared with the device code.  Float64 throughout; sums in numpy's own order."""
import numpy as np

U = 2.0 ** -53
RUNNING, CONVERGED, MAX_ITER, BREAKDOWN = "running", "converged", "max_iter", "breakdown"


class Graph:
    """the simple graph: src, dst the off-diagonal arcs in both directions sorted by (src, dst); loop, d, c per node;
    label[i] the smallest node of i's component in the loop-free graph"""

    def __init__(self, ptr, nbr):
        ptr, nbr = np.asarray(ptr, dtype=np.int64), np.asarray(nbr, dtype=np.int64)
        n = self.n = len(ptr) - 1
        row = np.repeat(np.arange(n, dtype=np.int64), np.diff(ptr))
        lo, hi = np.minimum(row, nbr), np.maximum(row, nbr)
        key = np.unique(lo * n + hi)
        lo, hi = key // n, key % n
        self.loop = np.zeros(n, dtype=np.int64)
        self.loop[lo[lo == hi]] = 1
        off = lo != hi
        src, dst = np.concatenate([lo[off], hi[off]]), np.concatenate([hi[off], lo[off]])
        o = np.lexsort((dst, src))
        self.src, self.dst = src[o], dst[o]
        self.c = np.bincount(self.src, minlength=n).astype(np.int64)
        self.d = self.c + self.loop
        self.ptr = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(self.c, out=self.ptr[1:])
        self.invc = np.where(self.c > 0, 1.0 / np.maximum(self.c, 1), 0.0)
        self.label = self._components()
        self.roots, self.comp, self.size = np.unique(self.label, return_inverse=True, return_counts=True)

    def _components(self):
        lab = np.arange(self.n, dtype=np.int64)
        while True:
            new = lab.copy()
            if len(self.src):
                np.minimum.at(new, self.src, lab[self.dst])
            while True:
                j = new[new]
                if np.array_equal(j, new):
                    break
                new = j
            if np.array_equal(new, lab):
                return lab
            lab = new

    def nbr_sum(self, v):
        """sum of v over each node's neighbours j != i"""
        return np.bincount(self.src, weights=v[self.dst], minlength=self.n) if len(self.src) else np.zeros(self.n)

    def product(self, v):
        """K v, K = diag(c) - A_off"""
        return self.c * v - self.nbr_sum(v)

    def comp_sum(self, v):
        return np.bincount(self.comp, weights=v, minlength=len(self.roots))

    def dense_K(self):
        K = np.diag(self.c.astype(np.float64))
        K[self.src, self.dst] -= 1.0
        return K

    def dense_L(self):
        """I - D^-1 A as the reference builds it"""
        A = np.zeros((self.n, self.n))
        A[self.src, self.dst] = 1.0
        A[np.arange(self.n), np.arange(self.n)] = self.loop
        return np.identity(self.n) - A / self.d[:, None]


def rhs(G, r=None):
    """steps 2 and 3: b = d * (r - d * (sum_C d r / sum_C d^2))"""
    r = np.ones(G.n) if r is None else np.asarray(r, dtype=np.float64)
    d = G.d.astype(np.float64)
    s1 = G.comp_sum(d * r)
    s2 = np.zeros(len(G.roots), dtype=np.int64)                          # exact: d_i <= n < 2^31 and the graphs here are small
    np.add.at(s2, G.comp, G.d * G.d)
    return d * (r - d * (s1 / s2.astype(np.float64))[G.comp])


class PCG:
    """the iteration of the header, one step at a time; the state is x, res, p, rho, it"""

    def __init__(self, G, b, tol=1e-10, max_iter=10000):
        self.G, self.b, self.tol, self.max_iter = G, b, float(tol), int(max_iter)
        self.bnorm = float(np.sqrt(np.dot(b, b)))
        self.x = np.zeros(G.n)
        self.res = b.copy()
        self.p = self.res * G.invc
        self.rho = float(np.dot(self.res, self.p))
        self.it = 0
        self.status = CONVERGED if self.bnorm == 0.0 else RUNNING
        self.last = {}

    def state(self):
        return {"x": self.x.copy(), "res": self.res.copy(), "p": self.p.copy(), "rho": self.rho, "it": self.it}

    def step(self):
        """one iteration; True once the run has stopped"""
        if self.status != RUNNING:
            return True
        G = self.G
        q = G.product(self.p)
        pq = float(np.dot(self.p, q))
        if not (pq > 0.0) or not np.isfinite(pq):
            self.status = BREAKDOWN
            return True
        alpha = self.rho / pq
        self.x = self.x + alpha * self.p
        self.res = self.res - alpha * q
        z = self.res * G.invc
        rho = float(np.dot(self.res, z))
        beta = rho / self.rho
        p_old = self.p
        self.p = z + beta * self.p
        self.last = {"q": q, "pq": pq, "alpha": alpha, "beta": beta, "z": z, "p_old": p_old, "rho_old": self.rho}
        self.rho = rho
        self.it += 1
        self.rr = float(np.dot(self.res, self.res))
        if np.sqrt(self.rr) <= self.tol * self.bnorm:
            self.status = CONVERGED
        elif self.it >= self.max_iter:
            self.status = MAX_ITER
        return self.status != RUNNING

    def run(self, trace=None):
        """to the stop; trace: a list that receives the state before every iteration"""
        while self.status == RUNNING:
            if trace is not None:
                trace.append(self.state())
            self.step()
        return self

    def true_residual(self):
        t = self.b - self.G.product(self.x)
        return float(np.sqrt(np.dot(t, t))) / self.bnorm if self.bnorm > 0 else 0.0


def centre(G, x):
    """step 5: x less its mean over each component"""
    return x - (G.comp_sum(x) / G.size)[G.comp]


def potential(ptr, nbr, r=None, tol=1e-10, max_iter=10000):
    """(V, info) as nabo_amd.diff_potential_csr returns them"""
    G = Graph(ptr, nbr)
    s = PCG(G, rhs(G, r), tol, max_iter).run()
    return centre(G, s.x), {"iterations": s.it, "status": s.status, "true_residual": s.true_residual(), "n_components": len(G.roots)}


def best_attainable(G, b, max_iter=None):
    """the iterate of smallest true residual the recurrence reaches with tol = 0: (x, its true relative residual)"""
    s = PCG(G, b, 0.0, max_iter or min(10000, 4 * G.n + 50))
    best, best_t = s.x.copy(), s.true_residual()
    while s.status == RUNNING:
        s.step()
        t = s.true_residual()
        if t < best_t:
            best, best_t = s.x.copy(), t
    return best, best_t


def pinv_potential(G, r=None):
    """the reference's route: numpy.linalg.pinv(I - A/D) r"""
    r = np.ones(G.n) if r is None else np.asarray(r, dtype=np.float64)
    return np.dot(np.linalg.pinv(G.dense_L()), r)


def lambda2(G):
    """the smallest non-zero eigenvalue of K: K has one zero eigenvalue per component"""
    ev = np.linalg.eigvalsh(G.dense_K())
    nc = len(G.roots)
    return float(ev[nc]) if nc < G.n else float("inf")


# ---- the bounds the tests hold one iteration to -----------------------------------------------------------------------
def row_bound(G, v):
    """per row, how far two float64 evaluations of (K v)_i can lie apart: (c_i + 1) u (c_i |v_i| + sum_j |v_j|) each"""
    return 2.0 * (G.c + 1) * U * (G.c * np.abs(v) + G.nbr_sum(np.abs(v)))


def dot_bound(a, b):
    """how far two float64 evaluations of a^T b can lie apart: n u sum |a_i b_i| each"""
    return 2.0 * len(a) * U * float(np.abs(a * b).sum())


# ---- graphs ---------------------------------------------------------------------------------------------------------
def csr_of_edges(n, edges):
    """edges: (i, j) in listing order, each listed once from i"""
    rows = [[] for _ in range(n)]
    for i, j in edges:
        rows[i].append(j)
    ptr = np.zeros(n + 1, dtype=np.int64)
    ptr[1:] = np.cumsum([len(r) for r in rows])
    return ptr, np.array([j for r in rows for j in r], dtype=np.int64)


def path_graph(n):
    return csr_of_edges(n, [(i, i + 1) for i in range(n - 1)])


def hub_graph(long_threshold):
    """a ring of long_threshold + 300 nodes and a hub joined to all of them; two more nodes joined to exactly
    long_threshold and long_threshold + 1 ring nodes: rows on either side of the threshold"""
    m = long_threshold + 300
    edges = [(i, (i + 1) % m) for i in range(m)] + [(m, i) for i in range(m)]
    edges += [(m + 1, 2 * i) for i in range(long_threshold)] + [(m + 2, i) for i in range(long_threshold + 1)]
    return csr_of_edges(m + 3, edges)


def kites_graph(count):
    """`count` components of 9 nodes each, a clique of 8 with a pendant node: well conditioned (a handful of distinct
    eigenvalues, so a handful of iterations) however many nodes there are"""
    edges = []
    for k in range(count):
        o = 9 * k
        edges += [(o + i, o + j) for i in range(8) for j in range(i + 1, 8)] + [(o + 8, o)]
    return csr_of_edges(9 * count, edges)


def small_graphs():
    g = {}
    g["one_loop"] = csr_of_edges(1, [(0, 0)])
    g["pair"] = csr_of_edges(2, [(0, 1)])
    g["loop_beside_clique"] = csr_of_edges(6, [(0, 0)] + [(i, j) for i in range(1, 6) for j in range(i + 1, 6)] + [(3, 3)])
    return g
