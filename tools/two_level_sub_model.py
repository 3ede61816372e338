"""CPU model of the two-level stream with a SUB-ORDER inside the buckets: tools/two_level_model.py with the
number of buckets C, the sub-anchors per bucket S and their ranking as parameters.  numpy only, float64, no GPU.
    python tools/two_level_sub_model.py [n] [waves]        (default 200000 x 200000, d = 50, 24 waves)
Both sides are sorted by (bucket, rank of the nearest sub-anchor, caller order) -- the rule of nabo_amd/csrc/local_seeds.h in
float64: the sub-anchors of a bucket are its references number j * (count / S) in caller order, ranked along their first
principal direction (power iteration from the all-ones vector, 8 steps) or by index; a bucket with fewer than S references
keeps caller order.  The seeds stay what they are: the 23rd smallest over the first 16384 cells, in CALLER order, of the
wave's own bucket among `seed_C` = 64 buckets, whatever C the stream is ordered by."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nabo_amd._synth import pca_like  # noqa: E402


def d2(P, Q):
    return np.maximum((P * P).sum(1)[:, None] + (Q * Q).sum(1)[None] - 2 * P @ Q.T, 0)


def sub_ranks(A, by_index):
    S = len(A)
    if by_index:
        return np.arange(S)
    Z = A - A.mean(0)
    v = np.ones(A.shape[1])
    for _ in range(8):
        w = Z.T @ (Z @ v)
        ss = float(w @ w)
        if not 0.0 < ss < np.inf:
            break
        v = w / np.sqrt(ss)
    return np.argsort(np.argsort(Z @ v, kind="stable"), kind="stable")


def order(Y, X, C, S, by_index):
    """the permutations of both sides and the references' buckets"""
    n = len(Y)
    A = Y[:: n // C][:C]
    bY, bX = d2(Y, A).argmin(1), d2(X, A).argmin(1)
    rY, rX = np.zeros(len(Y), dtype=np.int64), np.zeros(len(X), dtype=np.int64)
    for b in range(C):
        iy, ix = np.flatnonzero(bY == b), np.flatnonzero(bX == b)
        if S <= 1 or len(iy) < S:
            continue
        sub = Y[iy[np.arange(S) * (len(iy) // S)]]
        rank = sub_ranks(sub, by_index)
        rY[iy] = rank[d2(Y[iy], sub).argmin(1)]
        if len(ix):
            rX[ix] = rank[d2(X[ix], sub).argmin(1)]
    return np.lexsort((rY, bY)), np.lexsort((rX, bX)), bY, bX             # (lexsort is stable: caller order last)


def run(name, Y, X, C=64, S=1, by_index=False, head=28, L=23, nw=24, seed_C=64):
    n, m = len(Y), len(X)
    oy, ox, _, _ = order(Y, X, C, S, by_index)
    A0 = Y[:: n // seed_C][:seed_C]
    sY, sX = d2(Y, A0).argmin(1), d2(X, A0).argmin(1)                      # the seeds' buckets: always seed_C, caller order
    Yo, nt = Y[oy], n // 32
    Yh, Yt = Yo[:, :head], np.linalg.norm(Yo[:, head:], axis=1)
    rng = np.random.default_rng(1)
    fin, seed_share = [], []
    for w in rng.choice(m // 96, nw, replace=False):
        rows = ox[w * 96:(w + 1) * 96]
        Xw = X[rows]
        full = d2(Xw, Yo)
        tau = np.partition(full, L - 1, axis=1)[:, L - 1]
        own = d2(Xw, Y[sY == np.bincount(sX[rows]).argmax()][:16384])
        seed = np.partition(own, L - 1, axis=1)[:, L - 1] if own.shape[1] >= L else np.full(96, np.inf)
        lb1 = d2(Xw[:, :head], Yh) + (np.linalg.norm(Xw[:, head:], axis=1)[:, None] - Yt[None]) ** 2
        for t, out in ((tau, fin), (seed, seed_share)):
            out.append((lb1 < t[:, None])[:, :nt * 32].reshape(96, nt, 32).any(axis=(0, 2)).mean())
    print("| %s | %.2f %% | %.2f %% | %.0f %% |" % (name, 100 * np.mean(seed_share), 100 * np.mean(fin), 100 * np.max(seed_share)), flush=True)


if __name__ == "__main__":
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 200000
    nw = int(sys.argv[2]) if len(sys.argv) > 2 else 24
    Y, X = pca_like(n, 50, 1003), pca_like(n, 50, 2003)
    print("| order of both sides (%d x %d, %d waves) | tiles needing step 1, seed thresholds | final thresholds | worst wave |" % (n, n, nw))
    print("|---|---|---|---|")
    run("64 buckets, caller order inside", Y, X, nw=nw)
    run("256 flat buckets", Y, X, C=256, nw=nw)
    for S in (8, 16, 32, 64):
        run("64 buckets x %d sub-anchors, ranked along their direction" % S, Y, X, S=S, nw=nw)
    for S in (8, 32):
        run("64 buckets x %d sub-anchors, ranked by index" % S, Y, X, S=S, by_index=True, nw=nw)
