"""Plain float64 numpy restatement of include/nabo_umap.h, parts A to D (part E lives in nabo_amd/_umap.py and is host
code already), and the inputs the UMAP tests run on.  Everything is literal: the sums are taken in the header's order
(binary trees over padded slots, the 256 strided accumulators, lane by lane and round by round within a node's row), with
loops where the order matters.  Beside each result it returns what the tests' bounds scale with: the rows whose sigma
search came close to a comparison's threshold, the arcs close to the prune threshold, the sums of absolute terms."""
import numpy as np

M64 = (1 << 64) - 1
GOLD = 0x9E3779B97F4A7C15
NEAR = 1e-12          # a comparison of the sigma search closer to its threshold than this is flagged
W_TOL = 16 * 2.0 ** -53
# |w_gpu - w_ref| <= W_TOL: rho and sigma are bit-equal and x / sigma is one IEEE division, so a = exp(-(x / sigma))
# differs only by the two exp: the device's (1 ulp documented for HIP's double exp, 2 allowed here) plus numpy's (below
# 1 ulp); a <= 1, so |da| <= 3 * 2^-53.  w = (a + b) - a b with a, b in [0, 1]: |dw| <= |da| + |db| + three roundings of
# values <= 2, i.e. at most (6 + 6) 2^-53, rounded up to 16 * 2^-53.
TERM_ULPS = 32
# relative error allowed between the device's and numpy's value of one term c * D of an epoch: D is exact (the same
# IEEE subtraction of the same positions), c takes at most two pow (device: 1 ulp documented, 2 allowed; numpy: up to 4
# in its vectorised loops) = 12, the denominator a p + 1 inherits no more than p's, and five further roundings on each
# side (two multiplications, the addition, the division, c * D) = 5: 17 ulp, rounded up to 32.


def mix(z):
    """the header's mix() on a uint64 array, wrapping"""
    z = np.atleast_1d(np.asarray(z, dtype=np.uint64))
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def mix_int(z):
    """the same on one Python integer"""
    z &= M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def sample(seed, t, e, p, n):
    """k' of sample p of arc e in epoch t, from the definition, in Python integers"""
    s_t = mix_int(seed + GOLD * (t + 1))
    s_e = mix_int(s_t + GOLD * (e + 1))
    z = mix_int(s_e + GOLD * (p + 1))
    return ((z >> 32) * n) >> 32


def tree_sum(v):
    """TREE of the header along the last axis: slots padded with 0 to a power of two, adjacent slots added, repeatedly"""
    v = np.asarray(v, dtype=np.float64)
    k = v.shape[-1]
    W = 1
    while W < k:
        W *= 2
    if W > k:
        v = np.concatenate([v, np.zeros(v.shape[:-1] + (W - k,))], axis=-1)
    while v.shape[-1] > 1:
        v = v[..., 0::2] + v[..., 1::2]
    return v[..., 0]


def total_sum(rowsum):
    """256 accumulators, accumulator c taking rows c, c + 256, ... in ascending order, then added by halving"""
    n = len(rowsum)
    pad = np.concatenate([rowsum, np.zeros(-n % 256)]).reshape(-1, 256)
    acc = np.zeros(256)
    for chunk in pad:
        acc = acc + chunk
    h = 128
    while h:
        acc[:h] = acc[:h] + acc[h:2 * h]
        h //= 2
    return float(acc[0])


def knn_lists(X, k):
    """part A by brute force: (dist asc, idx asc), the cell itself included"""
    X = np.asarray(X, dtype=np.float64)
    d = np.sqrt(((X[:, None, :] - X[None, :, :]) ** 2).sum(axis=2))
    order = np.argsort(d, axis=1, kind="stable")[:, :k]
    return order.astype(np.int64), np.take_along_axis(d, order, axis=1)


def smooth(dist):
    """part B: rho, sigma, and per row whether some comparison of the search came within NEAR of its threshold (rows whose
    psum holds an exp term: the others compare whole numbers), whether the floor acted, and psum at the sigma the search
    returned"""
    dist = np.asarray(dist, dtype=np.float64)
    n, k = dist.shape
    target = float(np.log2(k))
    pos = dist > 0
    rho = np.where(pos.any(axis=1), np.where(pos, dist, np.inf).min(axis=1), 0.0)
    x = dist - rho[:, None]

    def psum(mid):
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            v = np.where(x > 0, np.exp(-(x / mid[:, None])), 1.0)
        v[:, 0] = 0.0
        return tree_sum(v)

    lo, hi, mid = np.zeros(n), np.full(n, np.inf), np.ones(n)
    done, flagged = np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
    inexact = (x[:, 1:] > 0).any(axis=1)      # without an exp term psum is a whole number, the same everywhere
    for _ in range(64):
        p = psum(mid)
        act = ~done
        flagged |= act & inexact & ((np.abs(p - target) < NEAR) | (np.abs(p - (target + 1e-5)) < NEAR) | (np.abs(p - (target - 1e-5)) < NEAR))
        stop = act & (np.abs(p - target) < 1e-5)
        done |= stop
        up = act & ~stop & (p > target)
        dn = act & ~stop & ~(p > target)
        hi = np.where(up, mid, hi)
        lo = np.where(dn, mid, lo)
        with np.errstate(invalid="ignore"):
            half = (lo + hi) / 2.0
        mid = np.where(up, half, np.where(dn, np.where(np.isinf(hi), mid * 2.0, half), mid))
        if done.all():
            break
    psum_at = psum(mid)
    rowsum = tree_sum(dist)
    mean = np.where(rho > 0, rowsum / float(k), total_sum(rowsum) / (float(n) * float(k)))
    floor = 1e-3 * mean
    sigma = np.maximum(mid, floor)
    return rho, sigma, flagged, mid < floor, psum_at


def fuzzy_graph(idx, dist, n_epochs):
    """parts B and C.  dict: rho, sigma, ptr, nbr, w (pruned CSR), wmax, n_unpruned (arcs of positive weight: an exp
    that underflows to 0 leaves no arc, the prune drops it for every n_epochs), flagged (rows, part B), floored,
    psum_at, near (arcs of the unpruned graph within 2 W_TOL of the prune threshold)"""
    idx, dist = np.asarray(idx, dtype=np.int64), np.asarray(dist, dtype=np.float64)
    n, k = idx.shape
    rho, sigma, flagged, floored, psum_at = smooth(dist)
    x = dist - rho[:, None]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        a = np.where((x <= 0) | (sigma[:, None] == 0), 1.0, np.exp(-(x / sigma[:, None])))
    a[idx == np.arange(n)[:, None]] = 0.0
    memb = {}
    for i in range(n):
        for t in range(k):
            j = int(idx[i, t])
            if j != i:
                memb[(i, j)] = float(a[i, t])
    arcs = {}
    for (i, j), aij in memb.items():
        aji = memb.get((j, i), 0.0)
        w = (aij + aji) - aij * aji
        arcs[(i, j)] = w
        arcs[(j, i)] = w
    keys = sorted(arcs)
    src = np.array([p[0] for p in keys], dtype=np.int64)
    dst = np.array([p[1] for p in keys], dtype=np.int64)
    w = np.array([arcs[p] for p in keys], dtype=np.float64)
    wmax = float(w.max())
    thr = wmax / float(n_epochs)
    keep = ~(w < thr)
    near = np.abs(w - thr) <= 2 * W_TOL       # the device's wmax, hence its threshold, may be off by W_TOL too
    ptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(src[keep], minlength=n), out=ptr[1:])
    return dict(rho=rho, sigma=sigma, ptr=ptr, nbr=dst[keep], w=w[keep], wmax=wmax, n_unpruned=int((w > 0).sum()), flagged=flagged,
                floored=floored, psum_at=psum_at, near=near, all_src=src, all_dst=dst, all_w=w)


def clip(v):
    return np.where(v > 4.0, 4.0, np.where(v < -4.0, -4.0, v))


class Epochs:
    """part D on a pruned CSR: the schedule's state and one synchronous epoch at a time"""

    def __init__(self, ptr, nbr, w, wmax, n_epochs, negative_sample_rate, repulsion_strength, a, b, seed, group):
        self.ptr, self.nbr = np.asarray(ptr, dtype=np.int64), np.asarray(nbr, dtype=np.int64)
        self.n, self.E = len(self.ptr) - 1, len(self.nbr)
        self.n_epochs, self.nsr, self.seed, self.group = int(n_epochs), int(negative_sample_rate), int(seed), int(group)
        self.a, self.b = float(a), float(b)
        self.ca, self.cr = (-2.0 * self.a) * self.b, (2.0 * float(repulsion_strength)) * self.b
        self.eps = float(wmax) / np.asarray(w, dtype=np.float64)
        self.epn = self.eps / float(self.nsr)
        self.src = np.repeat(np.arange(self.n, dtype=np.int64), np.diff(self.ptr))
        rowpos = np.arange(self.E, dtype=np.int64) - self.ptr[self.src]
        self.lane, self.round = rowpos % self.group, rowpos // self.group
        self.rewind()

    def rewind(self):
        self.next, self.nneg, self.t = self.eps.copy(), self.epn.copy(), 0

    def firing(self):
        """(arcs that fire in epoch t, their numbers of negative samples), and the schedule moved on to t + 1"""
        tf = float(self.t)
        e = np.nonzero(self.next <= tf)[0]
        m = np.trunc((tf - self.nneg[e]) / self.epn[e]).astype(np.int64)
        self.next[e] = self.next[e] + self.eps[e]
        self.nneg[e] = self.nneg[e] + m.astype(np.float64) * self.epn[e]
        self.t += 1
        return e, m

    def advance(self, t):
        """the schedule alone up to epoch t: it does not depend on the positions"""
        while self.t < t:
            self.firing()

    def samples(self, t, e, p):
        """k' of sample p of the arcs e in epoch t (uint64 array)"""
        s_t = mix_int(self.seed + GOLD * (t + 1))
        with np.errstate(over="ignore"):
            s_e = mix(np.uint64(s_t) + np.uint64(GOLD) * (e.astype(np.uint64) + np.uint64(1)))
            z = mix(s_e + np.uint64((GOLD * (p + 1)) & M64))
        return ((z >> np.uint64(32)) * np.uint64(self.n)) >> np.uint64(32)

    def step(self, y):
        """one epoch from the positions y [n, dims]; dict: y (new), n_attr, n_neg, idx_sum, abs_terms (per node and
        component, the sum of |term|), n_terms, self_hits, clipped, terms"""
        y = np.asarray(y, dtype=np.float64)
        n, dims, G = self.n, y.shape[1], self.group
        t = self.t
        alpha = 1.0 - float(t) / float(self.n_epochs)
        e_all, m_all = self.firing()
        acc = np.zeros((n, G, dims))
        abs_terms = np.zeros((n, dims))
        n_attr, n_neg = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
        idx_sum = np.zeros(n, dtype=np.uint64)
        n_terms = np.zeros(n, dtype=np.int64)
        self_hits = clipped = terms = 0

        def d2_of(D):
            d2 = D[:, 0] * D[:, 0]
            for c in range(1, dims):
                d2 = d2 + D[:, c] * D[:, c]
            return d2

        for r in np.unique(self.round[e_all]):                 # a lane meets its arcs in row order: round by round
            sel = self.round[e_all] == r
            e, m = e_all[sel], m_all[sel]
            i, j, l = self.src[e], self.nbr[e], self.lane[e]
            D = y[i] - y[j]
            d2 = d2_of(D)
            with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                c = np.where(d2 > 0, (self.ca * np.power(d2, self.b - 1.0)) / (self.a * np.power(d2, self.b) + 1.0), 0.0)
            raw = c[:, None] * D
            g = 2.0 * clip(raw)
            acc[i, l] = acc[i, l] + g
            np.add.at(abs_terms, i, np.abs(g))
            np.add.at(n_attr, i, 1)
            np.add.at(n_terms, i, 1)
            clipped += int((np.abs(raw) > 4.0).any(axis=1).sum())
            terms += len(e)
            for p in range(int(m.max()) if len(m) else 0):
                has = m > p
                ep, ip, lp = e[has], i[has], l[has]
                kk = self.samples(t, ep, p)
                np.add.at(n_neg, ip, 1)
                with np.errstate(over="ignore"):
                    np.add.at(idx_sum, ip, kk)
                kk = kk.astype(np.int64)
                other = kk != ip
                self_hits += int((~other).sum())
                ep, ip, lp, kk = ep[other], ip[other], lp[other], kk[other]
                D = y[ip] - y[kk]
                d2 = d2_of(D)
                with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                    c = np.where(d2 > 0, self.cr / ((0.001 + d2) * (self.a * np.power(d2, self.b) + 1.0)), 0.0)
                raw = c[:, None] * D
                g = clip(raw)
                acc[ip, lp] = acc[ip, lp] + g
                np.add.at(abs_terms, ip, np.abs(g))
                np.add.at(n_terms, ip, 1)
                clipped += int((np.abs(raw) > 4.0).any(axis=1).sum())
                terms += len(ep)
        S = tree_sum(np.moveaxis(acc, 1, 2))                   # [n, dims]: the lanes by the binary tree
        return dict(y=y + alpha * S, S=S, alpha=alpha, n_attr=n_attr, n_neg=n_neg, idx_sum=idx_sum, abs_terms=abs_terms,
                    n_terms=n_terms, self_hits=self_hits, clipped=clipped, terms=terms, fired=e_all, m=m_all)


def position_bound(o, y_old):
    """per node and component, what |y_gpu - y_ref| may be after one epoch from the same positions: every term within
    TERM_ULPS ulp of the restatement's (clipping does not enlarge a difference), the node's sum of n_terms terms
    reassociated at most once per addition, and the move's multiplication and addition"""
    u = 2.0 ** -53
    sum_err = (TERM_ULPS + o["n_terms"][:, None] + 8) * u * o["abs_terms"]
    return o["alpha"] * sum_err + 4 * u * (np.abs(y_old) + o["alpha"] * o["abs_terms"])


def neighbour_share(Y, X, near=10, wide=30):
    """(the mean share of a cell's `near` nearest embedded neighbours that are among its `wide` nearest in the input,
    the embedded neighbour lists [n, near])"""
    ie, _ = knn_lists(Y, near + 1)
    ii, _ = knn_lists(X, wide + 1)
    n = len(Y)
    hit = 0
    for c in range(n):
        hit += len(set(ie[c, 1:].tolist()) & set(ii[c, 1:].tolist()))
    return hit / float(n * near), ie[:, 1:]


def run(X, k, dims, n_epochs, a, b, seed, y0, group, negative_sample_rate=5, repulsion_strength=1.0):
    """the whole of A to D on the cells X from the start y0 (already scaled)"""
    idx, dist = knn_lists(X, k)
    g = fuzzy_graph(idx, dist, n_epochs)
    ep = Epochs(g["ptr"], g["nbr"], g["w"], g["wmax"], n_epochs, negative_sample_rate, repulsion_strength, a, b, seed, group)
    y = np.array(y0, dtype=np.float64)
    for _ in range(n_epochs):
        y = ep.step(y)["y"]
    return y


# ---------------------------------------------------------------------------------------------------------------------
# inputs

def blobs():
    """the whole-run data: 300 cells in 6 Gaussian groups of 50 in 12 dimensions, rotated onto their principal axes"""
    rng = np.random.default_rng(11)
    centres = rng.normal(0.0, 2.5, size=(6, 12))
    group = np.repeat(np.arange(6), 50)
    X = centres[group] + rng.normal(0.0, 1.0, size=(300, 12))
    X = X - X.mean(axis=0)
    _, _, vt = np.linalg.svd(X, full_matrices=False)
    return np.ascontiguousarray(X @ vt.T), group


def _points_case(n, k, seed, g=3, dup=None):
    X = np.random.default_rng(seed).normal(size=(n, g))
    if dup:
        for src, copies in dup:
            for c in copies:
                X[c] = X[src]
    return knn_lists(X, k)


def graph_cases():
    """name -> (idx, dist): the lists the graph tests run on (tests/test_umap_gpu.py case 1)"""
    cases = {}
    cases["knn_40x5"] = _points_case(40, 5, 1)
    cases["knn_333x15"] = _points_case(333, 15, 2, g=5)
    cases["knn_50x2"] = _points_case(50, 2, 3)
    cases["knn_120x56"] = _points_case(120, 56, 4, g=6)
    # cells 10..14 coincide (k = 5: their rows are all zero, rho = 0, the global-mean floor), 20 = 21 and 30 = 31 = 32
    # (zeros beyond position 0)
    cases["duplicates_60x5"] = _points_case(60, 5, 5, dup=[(10, (11, 12, 13, 14)), (20, (21,)), (30, (31, 32))])
    # hand-made rows: three entries tie at rho, so psum >= 3 > log2(5) whatever sigma is and the floor acts
    idx, dist = _points_case(40, 5, 6)
    for r in (7, 19):
        dist[r, 1:4] = dist[r, 1]
    cases["floor_40x5"] = (idx, dist)
    # every list names node 0: its row has 599 arcs, longer than a wavefront and than 256
    n, k = 600, 4
    rng = np.random.default_rng(7)
    idx = np.zeros((n, k), dtype=np.int64)
    dist = np.zeros((n, k))
    for i in range(n):
        if i == 0:
            idx[i] = [0, 1, 2, 3]
        else:
            others = [x for x in ((i + 1) % n, (i + 2) % n, (i + 3) % n) if x not in (0, i)][:2]
            idx[i] = [i, 0] + others
        dist[i, 1:] = np.sort(rng.uniform(0.5, 2.0, size=k - 1))
    cases["hub_600x4"] = (idx, dist)
    return cases


WIDTH_K = (8, 9, 16, 17, 30, 32, 33)


def width_cases():
    """name -> (idx, dist): lists that fill a width of the graph kernels (8, 16, 32), sit one above one (9, 17, 33), and
    the usual k = 30.  Kept apart from graph_cases(), whose names tests/golden/umap.npz pins"""
    return {"knn_%dx%d" % (200 + 10 * at, k): _points_case(200 + 10 * at, k, 11 + at, g=6) for at, k in enumerate(WIDTH_K)}


def width_of(k):
    """the lanes a row of k entries takes in the graph kernels (umap_width in nabo_amd/csrc/umap.hip)"""
    return 8 if k <= 8 else 16 if k <= 16 else 32 if k <= 32 else 64


N_EPOCHS_PRUNING, N_EPOCHS_KEEPING = 8, 10 ** 9
