"""A numpy model of the one-product filter's list work on the headline stream: how many list updates a target row
makes over the bench's references, in the caller's order, with lists of 23 -- from +inf, from today's tournament seed
(the 23rd smallest score of the stream's first 1035 tiles), and from a seed taken over the row's own bucket of a
partition of the references (local tournament seeds).  Exact float64 scores; the seed is the exact 23rd
smallest score of the sample (the tournament's group minima give a slightly higher bound).  CPU only.
    python tools/local_seed_model.py [rows] [n] [g]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nabo_amd._synth import pca_like  # noqa: E402

L = 23
rows = int(sys.argv[1]) if len(sys.argv) > 1 else 256
n = int(sys.argv[2]) if len(sys.argv) > 2 else 1000000
g = int(sys.argv[3]) if len(sys.argv) > 3 else 50
Y = pca_like(n, g, seed=1003)
X = pca_like(1000000, g, seed=2003)[:rows]
yn = (Y * Y).sum(1)


def scores(x):
    return yn - 2.0 * (Y @ x)                  # ||y||^2 - 2 x.y: the filter's score up to the row's constant


def nearest(P, A):
    d = (A * A).sum(1)[None, :] - 2.0 * (P @ A.T)
    return d.argmin(1)


def updates(d, seed):
    """insertions into a list of L entries that starts as L copies of `seed`, over the stream d"""
    kept = np.full(L, seed)
    tau, cnt = seed, 0
    for c0 in range(0, len(d), 8192):
        blk = d[c0:c0 + 8192]
        for j in np.flatnonzero(blk < tau):
            if blk[j] < tau:
                kept[kept.argmax()] = blk[j]
                tau = kept.max()
                cnt += 1
    return cnt


def partitions():
    yield "today (stream prefix, 1035 tiles)", None, None, None
    for C, cap in ((64, None), (64, 16384), (64, 4096), (256, 16384)):
        A = Y[::n // C][:C]
        yield "nearest of %d strided refs, cap %s" % (C, cap or "whole bucket"), nearest(Y, A), nearest(X, A), cap
    A = Y[::n // 64][:64].copy()
    for _ in range(4):                         # 64-means, 4 Lloyd steps from the strided anchors
        b = nearest(Y, A)
        for c in range(64):
            if (b == c).any():
                A[c] = Y[b == c].mean(0)
    yield "64-means, 4 Lloyd steps, whole bucket", nearest(Y, A), nearest(X, A), None
    mu = Y.mean(0)
    bits = lambda P: (((P[:, :6] - mu[:6]) > 0) * (1 << np.arange(6))).sum(1)      # noqa: E731
    yield "sign bits of 6 leading centred comps, cap 16384", bits(Y), bits(X), 16384


D = [scores(x) for x in X]
none = [updates(d, np.inf) for d in D]
print("no seeds: %.1f updates per row" % np.mean(none))
print("| partition | updates per row: mean / p90 / max |\n|---|---|")
for name, by, bx, cap in partitions():
    cnt = []
    for r, d in enumerate(D):
        if by is None:
            smp = d[:1035 * 32]
        else:
            smp = d[np.flatnonzero(by == bx[r])[:cap]]
        seed = np.partition(smp, L - 1)[L - 1] if len(smp) >= L else np.inf
        cnt.append(updates(d, seed))
    print("| %s | %.1f / %d / %d |" % (name, np.mean(cnt), np.percentile(cnt, 90), max(cnt)), flush=True)
