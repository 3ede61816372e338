"""Plain float64 numpy restatement of include/nabo_umap_transform.h, parts A' to D', and the inputs the transform tests
run on.  Everything is literal: TREE sums over padded slots, the start added in list order, a target's displacement lane
by lane and round by round, with loops where the order matters.  Beside each result it returns what the tests' bounds
scale with: the rows whose sigma search came close to a comparison's threshold, the sums of absolute terms."""
import numpy as np

import _umap_ref as ur
from _umap_ref import GOLD, M64, NEAR, TERM_ULPS, clip, mix, mix_int, position_bound, sample, tree_sum  # noqa: F401

U = 2.0 ** -53
MEMB_TOL = 3 * U
# |a_gpu - a_ref| <= MEMB_TOL: sigma is bit-equal and d / sigma is one IEEE division of the same operands, so
# a = exp(-(d / sigma)) differs only by the two exp: the device's (1 ulp documented for HIP's double exp, 2 allowed here)
# plus numpy's (below 1 ulp); a <= 1, where an ulp is at most 2^-53, so |da| <= 3 * 2^-53 (what W_TOL of _umap_ref
# starts from).


def start_bound(idx, memb, Y):
    """per target and component, what |y0_gpu - y0_ref| may be.  With da = MEMB_TOL, u = 2^-53, depth = log2 of TREE's
    width, all to first order and then enlarged by 1 % for the terms of second order:
      s = TREE(a), all terms >= 0: the two sides' inputs differ by at most k da in sum and each side rounds depth
          additions of partial sums <= s                                   |ds| <= k da + 2 depth u s
      w_t = a_t / s, one division on each side                             |dw_t| <= da / s + a_t |ds| / s^2 + 2 u w_t
      p_t = w_t * Y_t, one multiplication on each side                     |dp_t| <= |Y_t| |dw_t| + 2 u |p_t|
      y = the k products added in order from 0 (the first addition is exact), each side rounding k - 1 partial sums
          that are at most sum |p_t|                                       |dy| <= sum |dp_t| + 2 (k - 1) u sum |p_t|"""
    memb = np.asarray(memb, dtype=np.float64)
    k = memb.shape[1]
    depth = int(np.ceil(np.log2(k)))
    s = tree_sum(memb)[:, None]
    ds = k * MEMB_TOL + 2 * depth * U * s
    w = memb / s
    dw = MEMB_TOL / s + memb * ds / (s * s) + 2 * U * w
    absY = np.abs(np.asarray(Y, dtype=np.float64)[idx])                  # [m, k, dims]
    p = w[:, :, None] * absY
    dp = absY * dw[:, :, None] + 2 * U * p
    return 1.01 * (dp.sum(axis=1) + 2 * (k - 1) * U * p.sum(axis=1))


def knn_lists(Z, X, k):
    """part A' by brute force: each target's k nearest reference cells in (dist asc, idx asc) order"""
    Z, X = np.asarray(Z, dtype=np.float64), np.asarray(X, dtype=np.float64)
    d = np.sqrt(((Z[:, None, :] - X[None, :, :]) ** 2).sum(axis=2))
    order = np.argsort(d, axis=1, kind="stable")[:, :k]
    return order.astype(np.int64), np.take_along_axis(d, order, axis=1)


def smooth(dist):
    """part B': sigma, and per row whether some comparison of the search came within NEAR of its threshold (rows whose
    psum holds an exp term: the others compare whole numbers), whether the floor acted, and psum at the sigma the search
    returned"""
    dist = np.asarray(dist, dtype=np.float64)
    m, k = dist.shape
    target = float(np.log2(k))

    def psum(mid):
        with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
            v = np.where(dist > 0, np.exp(-(dist / mid[:, None])), 1.0)
        v[:, 0] = 0.0
        return tree_sum(v)

    lo, hi, mid = np.zeros(m), np.full(m, np.inf), np.ones(m)
    done, flagged = np.zeros(m, dtype=bool), np.zeros(m, dtype=bool)
    inexact = (dist[:, 1:] > 0).any(axis=1)
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
    floor = 1e-3 * (tree_sum(dist) / float(k))
    return np.maximum(mid, floor), flagged, mid < floor, psum_at


def memberships(dist, sigma):
    """part C': a [m, k]"""
    dist, sigma = np.asarray(dist, dtype=np.float64), np.asarray(sigma, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        return np.where((dist <= 0) | (sigma[:, None] == 0), 1.0, np.exp(-(dist / sigma[:, None])))


def start(idx, memb, Y):
    """the start: the products added in list order, starting from 0"""
    idx, memb, Y = np.asarray(idx, dtype=np.int64), np.asarray(memb, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    s = tree_sum(memb)
    with np.errstate(divide="ignore", invalid="ignore"):
        w = memb / s[:, None]
    y = np.zeros((idx.shape[0], Y.shape[1]))
    for t in range(idx.shape[1]):
        y = y + w[:, t, None] * Y[idx[:, t]]
    return y


def graph(idx, dist, Y):
    """parts B', C' and the start.  dict: sigma, memb, y0, flagged, floored, psum_at"""
    sigma, flagged, floored, psum_at = smooth(dist)
    memb = memberships(dist, sigma)
    return dict(sigma=sigma, memb=memb, y0=start(idx, memb, Y), flagged=flagged, floored=floored, psum_at=psum_at)


class Epochs:
    """part D' on one batch: the schedule's state and one epoch at a time.  Y is never written."""

    def __init__(self, idx, memb, Y, first_row, n_epochs, negative_sample_rate, repulsion_strength, a, b, seed, group):
        self.idx, self.memb = np.asarray(idx, dtype=np.int64), np.asarray(memb, dtype=np.float64)
        self.Y = np.asarray(Y, dtype=np.float64)
        self.m, self.k = self.idx.shape
        self.n_ref, self.first_row = len(self.Y), int(first_row)
        self.n_epochs, self.nsr, self.seed, self.group = int(n_epochs), int(negative_sample_rate), int(seed), int(group)
        self.a, self.b = float(a), float(b)
        self.ca, self.cr = (-2.0 * self.a) * self.b, (2.0 * float(repulsion_strength)) * self.b
        self.live = self.memb >= 1.0 / float(self.n_epochs)
        with np.errstate(divide="ignore"):
            self.eps = 1.0 / self.memb
        self.epn = self.eps / float(self.nsr)
        pos = np.arange(self.k, dtype=np.int64)
        self.lane, self.round = pos % self.group, pos // self.group
        self.rewind()

    def rewind(self):
        self.next, self.nneg, self.t = np.where(self.live, self.eps, np.inf), self.epn.copy(), 0

    def firing(self):
        """(rows, list positions, numbers of negative samples) of the arcs that fire in epoch t, and the schedule moved
        on to t + 1"""
        tf = float(self.t)
        i, tp = np.nonzero(self.next <= tf)
        m = np.trunc((tf - self.nneg[i, tp]) / self.epn[i, tp]).astype(np.int64)
        self.next[i, tp] = self.next[i, tp] + self.eps[i, tp]
        self.nneg[i, tp] = self.nneg[i, tp] + m.astype(np.float64) * self.epn[i, tp]
        self.t += 1
        return i, tp, m

    def advance(self, t):
        """the schedule alone up to epoch t: it does not depend on the positions"""
        while self.t < t:
            self.firing()

    def samples(self, t, i, tp, p):
        """k' of sample p of the arcs (i, tp) in epoch t (uint64 array)"""
        s_t = mix_int(self.seed + GOLD * (t + 1))
        e = ((self.first_row + i) * self.k + tp).astype(np.uint64)
        with np.errstate(over="ignore"):
            s_e = mix(np.uint64(s_t) + np.uint64(GOLD) * (e + np.uint64(1)))
            z = mix(s_e + np.uint64((GOLD * (p + 1)) & M64))
        return ((z >> np.uint64(32)) * np.uint64(self.n_ref)) >> np.uint64(32)

    def step(self, y):
        """one epoch from the targets' positions y [m, dims]; dict: y (new), alpha, n_attr, n_neg, idx_sum, abs_terms
        (per target and component, the sum of |term|), n_terms, clipped, terms, zero_d2"""
        y = np.asarray(y, dtype=np.float64)
        m, dims, G = self.m, y.shape[1], self.group
        t = self.t
        alpha = 0.25 * (1.0 - float(t) / float(self.n_epochs))
        i_all, tp_all, m_all = self.firing()
        acc = np.zeros((m, G, dims))
        abs_terms = np.zeros((m, dims))
        n_attr, n_neg, n_terms = np.zeros(m, dtype=np.int64), np.zeros(m, dtype=np.int64), np.zeros(m, dtype=np.int64)
        idx_sum = np.zeros(m, dtype=np.uint64)
        clipped = terms = zero_d2 = 0

        def d2_of(D):
            d2 = D[:, 0] * D[:, 0]
            for c in range(1, dims):
                d2 = d2 + D[:, c] * D[:, c]
            return d2

        for r in np.unique(self.round[tp_all]):                # a lane meets its arcs in list order: round by round
            sel = self.round[tp_all] == r
            i, tp, ms = i_all[sel], tp_all[sel], m_all[sel]
            l = self.lane[tp]
            D = y[i] - self.Y[self.idx[i, tp]]
            d2 = d2_of(D)
            zero_d2 += int((d2 == 0).sum())
            with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                c = np.where(d2 > 0, (self.ca * np.power(d2, self.b - 1.0)) / (self.a * np.power(d2, self.b) + 1.0), 0.0)
            raw = c[:, None] * D
            g = clip(raw)
            acc[i, l] = acc[i, l] + g                          # (within a round a target's arcs sit on distinct lanes)
            np.add.at(abs_terms, i, np.abs(g))
            np.add.at(n_attr, i, 1)
            np.add.at(n_terms, i, 1)
            clipped += int((np.abs(raw) > 4.0).any(axis=1).sum())
            terms += len(i)
            for p in range(int(ms.max()) if len(ms) else 0):
                has = ms > p
                ip, tpp, lp = i[has], tp[has], l[has]
                kk = self.samples(t, ip, tpp, p)
                np.add.at(n_neg, ip, 1)
                with np.errstate(over="ignore"):
                    np.add.at(idx_sum, ip, kk)
                D = y[ip] - self.Y[kk.astype(np.int64)]
                d2 = d2_of(D)
                with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                    c = np.where(d2 > 0, self.cr / ((0.001 + d2) * (self.a * np.power(d2, self.b) + 1.0)), 0.0)
                raw = c[:, None] * D
                g = clip(raw)
                acc[ip, lp] = acc[ip, lp] + g
                np.add.at(abs_terms, ip, np.abs(g))
                np.add.at(n_terms, ip, 1)
                clipped += int((np.abs(raw) > 4.0).any(axis=1).sum())
                terms += len(ip)
        S = tree_sum(np.moveaxis(acc, 1, 2))                   # [m, dims]: the lanes by the binary tree
        return dict(y=y + alpha * S, S=S, alpha=alpha, n_attr=n_attr, n_neg=n_neg, idx_sum=idx_sum, abs_terms=abs_terms,
                    n_terms=n_terms, clipped=clipped, terms=terms, zero_d2=zero_d2)


def run(Z, X, Y, k, n_epochs, a, b, seed, group, first_row=0, negative_sample_rate=5, repulsion_strength=1.0):
    """the whole of A' to D' for the targets Z against the reference cells X at the positions Y: (start, end)"""
    idx, dist = knn_lists(Z, X, k)
    g = graph(idx, dist, Y)
    ep = Epochs(idx, g["memb"], Y, first_row, n_epochs, negative_sample_rate, repulsion_strength, a, b, seed, group)
    y = g["y0"]
    for _ in range(n_epochs):
        y = ep.step(y)["y"]
    return g["y0"], y


def target_share(P, Y, Z, X, near=10, wide=30):
    """(the mean share of a target's `near` nearest embedded reference cells that are among its `wide` nearest reference
    cells in the input, the embedded lists [m, near])"""
    ie, _ = knn_lists(P, Y, near)
    ii, _ = knn_lists(Z, X, wide)
    hit = 0
    for c in range(len(P)):
        hit += len(set(ie[c].tolist()) & set(ii[c].tolist()))
    return hit / float(len(P) * near), ie


# ---------------------------------------------------------------------------------------------------------------------
# inputs

def held_out():
    """the whole-run data: _umap_ref.blobs() with 10 cells per group held out by default_rng(5):
    (reference rows, target rows), both ascending"""
    _, group = ur.blobs()
    rng = np.random.default_rng(5)
    tgt = np.sort(np.concatenate([rng.choice(np.nonzero(group == c)[0], size=10, replace=False) for c in range(6)]))
    ref = np.setdiff1d(np.arange(len(group)), tgt)
    return ref, tgt


def _case(n_ref, m, k, seed, g=3, dims=2, on_cell=(), dup=None):
    rng = np.random.default_rng(seed)
    X, Z = rng.normal(size=(n_ref, g)), rng.normal(size=(m, g))
    if dup:
        for src, copies in dup:
            for c in copies:
                X[c] = X[src]
    for row, cell in on_cell:
        Z[row] = X[cell]
    Y = rng.uniform(0.0, 10.0, size=(n_ref, dims))
    idx, dist = knn_lists(Z, X, k)
    return dict(idx=idx, dist=dist, Y=Y, X=X, Z=Z)


GROUP_K = (8, 9, 16, 32, 33, 48)


def list_cases():
    """name -> dict(idx, dist, Y, X, Z): the batches the graph tests run on.  k = 2, 5, 15, 17 and 56; m = 1, 17 and 333;
    then k = 8, 9, 16, 32, 33 and 48 (GROUP_K): a graph kernel's width filled and one over, and list lengths that are a
    multiple of the run kernel's group of 16 lanes or one over, 33 and 48 being three arcs to a lane"""
    cases = {}
    cases["k2_m17"] = _case(40, 17, 2, 101, dims=3)
    cases["k5_m1"] = _case(40, 1, 5, 102)
    # target 3 sits on reference cell 7: d_0 = 0
    cases["k15_m333"] = _case(600, 333, 15, 103, g=5, on_cell=[(3, 7)])
    cases["k17_m17"] = _case(100, 17, 17, 104, g=4, dims=3)
    cases["k56_m17"] = _case(120, 17, 56, 105, g=6)
    # reference cells 10..14 coincide and target 2 sits on them: all k = 5 distances are 0; cells 20 = 21 and target 5 on
    # them: zeros beyond position 0
    cases["zeros_k5_m17"] = _case(60, 17, 5, 106, on_cell=[(2, 10), (5, 20)], dup=[(10, (11, 12, 13, 14)), (20, (21,))])
    # a hand-made row: three entries tie
    c = _case(40, 17, 5, 107)
    c["dist"][9, 1:4] = c["dist"][9, 1]
    cases["ties_k5_m17"] = c
    for at, k in enumerate(GROUP_K):
        # k = 48: target 4 sits on reference cell 9, d_0 = 0 in the kernel of three arcs to a lane
        cases["k%d_m17" % k] = _case(200, 17, k, 110 + at, g=5, dims=2 + at % 2, on_cell=[(4, 9)] if k == 48 else ())
    return cases
