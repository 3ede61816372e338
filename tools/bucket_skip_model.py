"""How much of the two-level stream a unit of rows (a workgroup of 384 positions, or a wave of 96) can skip: the rule of
nabo_amd/csrc/bucket_skip.h in numpy, float64, on bench.py's data.  No GPU.
    python tools/bucket_skip_model.py [n] [units] [--unit 384|96] [--majority] [--oracle] [--sub S]
n references and as many targets (default 1 000 000), `units` sampled units (default 100).
  buckets: nearest of 64 strided references; 32 sub-anchors per bucket by the rule of local_seeds.h (references number
  j * (count // S) of the bucket, cells to the nearest, sub-anchors ranked along their first principal direction); both sides
  sorted by (bucket, sub-rank, caller order), reference buckets in whole tiles, target buckets in whole columns of 128;
  start thresholds: the 23rd smallest score among the first 16 384 references of the row's own bucket;
  the rule: hyperplane bound along the unit vector between the two buckets' MEANS, the minimum projection kept per reference
  sub-bucket, every row with the directions of its own bucket (--majority: of the unit's majority bucket, as the first
  model of this rule had it); kept sub-buckets widened to whole tiles and to pairs of tiles.
Prints the skipped share of the stream's tiles per unit (mean, median, p10, minimum), the kept runs per unit, and with
--oracle the share of (unit, sub-bucket) tiles that hold no reference below any row's threshold -- and checks on the way
that the rule skipped no (row, reference) pair below its row's threshold."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nabo_amd._synth import pca_like  # noqa: E402

args = sys.argv[1:]
flag = lambda f: f in args and not args.remove(f)      # noqa: E731
majority, oracle = flag("--majority"), flag("--oracle")


def value(f, default):
    if f not in args:
        return default
    i = args.index(f)
    args.pop(i)
    return int(args.pop(i))


unit, S = value("--unit", 384), value("--sub", 32)
n = int(args[0]) if args else 1000000
units = int(args[1]) if len(args) > 1 else 100
C, G, LKEEP, CAP = 64, 50, 23, 16384
Y, X = pca_like(n, G, seed=1003), pca_like(n, G, seed=2003)
centre = Y.mean(0)
Y, X = Y - centre, X - centre


def nearest(V, A, chunk=65536):
    an = (A * A).sum(1)
    return np.concatenate([np.argmin(an[None, :] - 2.0 * V[i:i + chunk] @ A.T, axis=1) for i in range(0, len(V), chunk)])


anchors = Y[np.arange(C) * (n // C)]
yb, xb = nearest(Y, anchors), nearest(X, anchors)
yr, xr = np.zeros(n, int), np.zeros(n, int)
for b in range(C):
    iy, ix = np.flatnonzero(yb == b), np.flatnonzero(xb == b)
    if len(iy) < S:
        continue
    A = Y[iy[np.arange(S) * (len(iy) // S)]]
    D = A - A.mean(0)
    v = np.ones(G)
    for _ in range(8):
        w = D.T @ (D @ v)
        if not 0 < w @ w < np.inf:
            break
        v = w / np.sqrt(w @ w)
    rank = np.argsort(np.argsort(D @ v, kind="stable"), kind="stable")
    yr[iy], xr[ix] = rank[nearest(Y[iy], A)], rank[nearest(X[ix], A)]
yo, xo = np.lexsort((np.arange(n), yr, yb)), np.lexsort((np.arange(n), xr, xb))
# reference positions: buckets in whole tiles; groups (bucket, rank) own the tiles first_touched .. last_touched
ycnt = np.bincount(yb, minlength=C)
ybase = np.concatenate([[0], np.cumsum((ycnt + 31) // 32 * 32)])
ypos = ybase[yb[yo]] + (np.arange(n) - np.concatenate([[0], np.cumsum(ycnt)])[yb[yo]])
tiles = (ybase[-1] // 32 + 1) // 2 * 2
gid = yb[yo] * S + yr[yo]                                  # group of every ordered reference: non-decreasing
gstart = np.searchsorted(gid, np.arange(C * S))
gend = np.searchsorted(gid, np.arange(C * S), side="right")
has = gend > gstart
t0 = np.where(has, ypos[np.minimum(gstart, n - 1)] // 32, 0)
t1 = np.where(has, ypos[np.maximum(gend - 1, 0)] // 32 + 1, 0)
mean = np.array([Y[yb == b].mean(0) if ycnt[b] else np.zeros(G) for b in range(C)])
# target positions: buckets in whole columns of 128, units of `unit` positions
xcnt = np.bincount(xb, minlength=C)
xbase = np.concatenate([[0], np.cumsum((xcnt + 127) // 128 * 128)])
xpos = xbase[xb[xo]] + (np.arange(n) - np.concatenate([[0], np.cumsum(xcnt)])[xb[xo]])
nunit = -(-xbase[-1] // unit)
Yo = Y[yo]
ymin_of = {}


def ymin(b):
    """[C * S]: the smallest projection of every group's references on the direction from bucket b to the group's bucket"""
    if b not in ymin_of:
        d = mean - mean[b]
        nrm = np.linalg.norm(d, axis=1)
        u = np.where((nrm > 0)[:, None], d / np.maximum(nrm, 1e-300)[:, None], 0.0)
        proj = np.einsum("ij,ij->i", Yo, u[yb[yo]])
        ymin_of[b] = (np.where(has, np.minimum.reduceat(proj, np.minimum(gstart, n - 1)), np.inf), u)
    return ymin_of[b]


rng = np.random.default_rng(1)
share, runs, oracle_free, oracle_all = [], [], 0, 0
for w in rng.choice(nunit, size=min(units, nunit), replace=False):
    rows = xo[(xpos >= w * unit) & (xpos < (w + 1) * unit)]
    if not len(rows):
        continue
    x, bx = X[rows], xb[rows]
    tau0 = np.empty(len(rows))
    for b in np.unique(bx):
        own = Y[np.flatnonzero(yb == b)[:CAP]]
        sc = (own * own).sum(1)[None, :] - 2.0 * x[bx == b] @ own.T
        tau0[bx == b] = np.partition(sc, LKEEP - 1, axis=1)[:, LKEEP - 1] if len(own) >= LKEEP else np.inf
    radius = np.sqrt(np.maximum(tau0 + (x * x).sum(1), 0.0))
    keep = np.zeros(C * S, bool)
    dirs = {int(np.bincount(bx).argmax())} if majority else set(int(b) for b in np.unique(bx))
    for b in dirs:
        ym, u = ymin(b)
        sel = slice(None) if majority else bx == b
        reach = (x[sel] @ u.T + radius[sel, None]).max(0)          # [C]: towards every bucket b'
        keep |= ~(ym >= np.repeat(reach, S))
    keep[np.repeat(np.isin(np.arange(C), np.unique(bx)), S)] = True
    keep &= has
    bits = np.zeros(tiles // 2, bool)
    for g in np.flatnonzero(keep):
        bits[t0[g] // 2:(t1[g] + 1) // 2] = True
    share.append(1.0 - bits.mean())
    runs.append(int((bits & ~np.concatenate([[False], bits[:-1]])).sum()))
    if oracle:
        sc = (Yo * Yo).sum(1)[None, :] - 2.0 * x @ Yo.T            # [rows, n]
        below = (sc < tau0[:, None]).any(0)
        grp_hit = np.add.reduceat(below, np.minimum(gstart, n - 1)) * has > 0
        assert not (grp_hit & ~keep).any(), "the rule skipped a pair below its row's threshold"
        tl = t1 - t0
        oracle_free += int(tl[has & ~grp_hit].sum())
        oracle_all += int(tl[has].sum())
share = np.array(share)
print("n = %d, %d units of %d positions, S = %d, %s directions" % (n, len(share), unit, S, "the majority bucket's" if majority else "each row's own"))
print("skipped share of the stream's tiles: mean %.1f %%, median %.1f %%, p10 %.1f %%, minimum %.1f %%" %
      (100 * share.mean(), 100 * np.median(share), 100 * np.percentile(share, 10), 100 * share.min()))
print("kept runs per unit: mean %.0f, at most %d" % (np.mean(runs), max(runs)))
if oracle:
    print("oracle: %.1f %% of the (unit, sub-bucket) tiles hold no reference below any row's threshold; no skipped pair lies below its row's threshold" %
          (100.0 * oracle_free / max(oracle_all, 1)))
