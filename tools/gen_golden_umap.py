#!/usr/bin/env python3
"""Writes tests/golden/umap.npz from the tests' float64 restatement of include/nabo_umap.h (tests/_umap_ref.py).

TEST INFRASTRUCTURE ONLY; runs on the CPU (the library is loaded for nabo_umap_geometry, which needs no device):

    python tools/gen_golden_umap.py [--out tests/golden/umap.npz]

Stored:
  * the whole-run data (300 cells in 6 Gaussian groups of 50 in 12 dimensions, on their principal axes) and, for seeds
    0-7, the "pca" and "random" starts and 2 and 3 dimensions, the restatement's result after 200 epochs with k = 15 as
    ONE figure each: the share of a cell's 10 nearest embedded neighbours that are among its 30 nearest in the input,
    and whether all 10 share the cell's group.  tests/test_umap_gpu.py demands of the device, per start and dimension,
    at least the minimum over the seeds minus their max-to-min spread;
  * for every list case of tests/_umap_ref.graph_cases and both n_epochs: the number of arcs and the sum of their
    weights, and the number of rows / arcs the restatement flags as too close to a threshold to pin (it must be 0: the
    cases are chosen so; this tool refuses to write otherwise);
  * for the four (spread, min_dist) of the curve test: the a, b of nabo_amd._umap.find_ab_params and, where scipy is
    installed, the largest difference between its curve and scipy.optimize.curve_fit's on the 300 points (NaN without
    scipy).  tests/test_umap_cpu.py allows 10 x that figure.
"""
import argparse
import datetime
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]

AB_CASES = [(1.0, 0.1), (1.0, 0.5), (2.0, 0.01), (0.5, 0.3)]
STARTS, DIMS, SEEDS = ("pca", "random"), (2, 3), tuple(range(8))
WHOLE_K, WHOLE_EPOCHS = 15, 200


def ab_curve_diff(spread, min_dist):
    """(a, b, the largest difference to scipy's fitted curve on the 300 points, or NaN without scipy)"""
    from nabo_amd import _umap
    a, b = _umap.find_ab_params(spread, min_dist)
    try:
        from scipy.optimize import curve_fit
    except ImportError:
        return a, b, float("nan")
    x, y = _umap.curve(spread, min_dist)
    f = lambda x, a, b: 1.0 / (1.0 + a * x ** (2 * b))    # umap's find_ab_params, word for word
    p, _ = curve_fit(f, x, y)
    return a, b, float(np.max(np.abs(f(x, a, b) - f(x, *p))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "umap.npz"))
    args = ap.parse_args()
    import _umap_ref as ur
    from nabo_amd import _umap
    group = _umap.geometry()

    names, n_arcs, w_sum, n_flagged = [], [], [], []
    for name, (idx, dist) in ur.graph_cases().items():
        for ne in (ur.N_EPOCHS_PRUNING, ur.N_EPOCHS_KEEPING):
            g = ur.fuzzy_graph(idx, dist, ne)
            names.append("%s/%d" % (name, ne))
            n_arcs.append(len(g["w"]))
            w_sum.append(float(g["w"].sum()))
            n_flagged.append(int(g["flagged"].sum()) + int(g["near"].sum()))
    assert not any(n_flagged), "a list case comes too close to a threshold: choose another seed (%s)" % dict(zip(names, n_flagged))

    ab = np.array([ab_curve_diff(s, m) for s, m in AB_CASES])

    X, grp = ur.blobs()
    a, b = _umap.find_ab_params(1.0, 0.1)
    share = np.zeros((len(STARTS), len(DIMS), len(SEEDS)))
    same_group = np.zeros(share.shape, dtype=bool)
    for si, start in enumerate(STARTS):
        for di, dims in enumerate(DIMS):
            for seed in SEEDS:
                y0 = _umap.start_positions(start, X, len(X), dims, seed)
                Y = ur.run(X, WHOLE_K, dims, WHOLE_EPOCHS, a, b, seed, y0, group)
                s, ie = ur.neighbour_share(Y, X)
                share[si, di, seed] = s
                same_group[si, di, seed] = bool((grp[ie] == grp[:, None]).all())
            print("%s start, %d dimensions: share %.4f .. %.4f, groups kept: %s"
                  % (start, dims, share[si, di].min(), share[si, di].max(), same_group[si, di].all()), flush=True)
    np.savez(args.out, blobs_X=X, blobs_group=grp, starts=np.array(STARTS), dims=np.array(DIMS, dtype=np.int64),
             seeds=np.array(SEEDS, dtype=np.int64), whole_k=np.int64(WHOLE_K), whole_epochs=np.int64(WHOLE_EPOCHS), share=share,
             same_group=same_group, start_share=np.array([ur.neighbour_share(_umap.start_positions("pca", X, len(X), 2, 0), X)[0],
                                                           ur.neighbour_share(_umap.start_positions("random", X, len(X), 2, 0), X)[0]]),
             graph_names=np.array(names), graph_n_arcs=np.array(n_arcs, dtype=np.int64), graph_w_sum=np.array(w_sum),
             graph_flagged=np.array(n_flagged, dtype=np.int64), ab_cases=np.array(AB_CASES), ab_fit=ab[:, :2], ab_curve_diff=ab[:, 2],
             group=np.int64(group), written=np.array(datetime.date.today().isoformat()))
    print("-> %s" % args.out)


if __name__ == "__main__":
    main()
