"""CPU model of the two-level stream of the one-product pass: which share of the (wave, tile) pairs needs the
second operand step when both sides are streamed in bucket order.  numpy only, float64, no GPU.
    python tools/two_level_model.py [n]                (default 200000 x 200000, d = 50: thresholds larger than at 1M, pessimistic)
Setup: bench.py's data; 64 anchors at stride n / 64, both sides sorted by nearest anchor; waves of 96 consecutive sorted rows,
tiles of 32 consecutive sorted references; LB1 = d^2(leading `head` components) + (||x_tail|| - ||y_tail||)^2, the first step's
bound up to the row's own norm; a tile needs the second step when LB1 < the row's threshold for any of its 96 x 32 pairs.
Thresholds: the local seeds (23rd smallest over the first 16384 cells of the wave's own bucket: where a list starts) and the
final ones (23rd smallest over all references: where it ends)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nabo_amd._synth import pca_like  # noqa: E402


def d2(P, Q):
    return np.maximum((P * P).sum(1)[:, None] + (Q * Q).sum(1)[None] - 2 * P @ Q.T, 0)


def run(name, n, m, d=50, head=28, C=64, L=23, nw=40, ordered=True, gen=pca_like):
    Y, X = gen(n, d, 1003), gen(m, d, 2003)
    A = Y[:: n // C][:C]
    bY, bX = d2(Y, A).argmin(1), d2(X, A).argmin(1)
    oy = np.argsort(bY, kind="stable") if ordered else np.arange(n)
    ox = np.argsort(bX, kind="stable") if ordered else np.arange(m)
    Yo, nt = Y[oy], n // 32
    Yh, Yt = Yo[:, :head], np.linalg.norm(Yo[:, head:], axis=1)
    rng = np.random.default_rng(1)
    fin, seed_share = [], []
    for w in rng.choice(m // 96, nw, replace=False):
        rows = ox[w * 96:(w + 1) * 96]
        Xw = X[rows]
        full = d2(Xw, Yo)
        tau = np.partition(full, L - 1, axis=1)[:, L - 1]
        own = full[:, bY[oy] == np.bincount(bX[rows]).argmax()][:, :16384]
        seed = np.partition(own, L - 1, axis=1)[:, L - 1] if own.shape[1] >= L else np.full(96, np.inf)
        lb1 = d2(Xw[:, :head], Yh) + (np.linalg.norm(Xw[:, head:], axis=1)[:, None] - Yt[None]) ** 2
        for t, out in ((tau, fin), (seed, seed_share)):
            out.append((lb1 < t[:, None])[:, :nt * 32].reshape(96, nt, 32).any(axis=(0, 2)).mean())
    print("| %s | %.1f %% | %.1f %% | %.0f %% |" % (name, 100 * np.mean(seed_share), 100 * np.mean(fin), 100 * np.max(seed_share)), flush=True)


def cloud(n, d, seed):
    """one broad Gaussian cloud with pca_like's component scales: no clusters"""
    return np.random.default_rng(seed).standard_normal((n, d)) * np.sqrt(30.0 - 29.0 * np.arange(d) / (d - 1))


if __name__ == "__main__":
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 200000
    print("| arrangement (%d x %d) | tiles needing the second step, seed thresholds | final thresholds | worst wave |" % (n, n))
    print("|---|---|---|---|")
    run("both sides bucket-ordered, 28 leading components", n, n)
    run("27 leading components", n, n, head=27)
    run("caller order", n, n, ordered=False, nw=10)
    run("one broad Gaussian cloud, bucket-ordered", n, n, gen=cloud, nw=10)
