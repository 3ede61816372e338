#!/usr/bin/env python3
"""Writes tests/golden/umap_transform.npz from the tests' float64 restatements of include/nabo_umap.h and
include/nabo_umap_transform.h (tests/_umap_ref.py, tests/_umap_transform_ref.py).

TEST INFRASTRUCTURE ONLY; runs on the CPU (the library is loaded for the two geometry calls, which need no device):

    python tools/gen_golden_umap_transform.py [--out tests/golden/umap_transform.npz]

Stored:
  * the held-out split of _umap_ref.blobs() (10 cells per group are targets, the other 240 the reference) and the
    reference's positions in 2 and 3 dimensions from _umap_ref.run (k = 15, 200 epochs, seed 0, the "pca" start);
  * for seeds 0-7 and both dimensions, the restatement's transform (k = 15, 100 epochs) as TWO figures each: the share of
    a target's 10 nearest embedded reference cells that are among its 30 nearest reference cells in the input, and
    whether all 10 are of the target's group; the same share for the start alone.  tests/test_umap_transform_gpu.py
    demands of the device, per dimension, at least the minimum over the seeds minus their max-to-min spread;
  * the restatement's positions for seed 0 in 2 dimensions, which tests/test_umap_transform_cpu.py reproduces;
  * the number of rows of tests/_umap_transform_ref.list_cases the restatement flags as too close to a threshold of
    the sigma search to pin (it must be 0: this tool refuses to write otherwise).
"""
import argparse
import datetime
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]

DIMS, SEEDS = (2, 3), tuple(range(8))
REF_K, REF_EPOCHS, REF_SEED = 15, 200, 0
WHOLE_K, WHOLE_EPOCHS = 15, 100


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "umap_transform.npz"))
    args = ap.parse_args()
    import _umap_ref as ur
    import _umap_transform_ref as tr
    from nabo_amd import _umap
    fit_group, group = _umap.geometry(), _umap.transform_geometry()

    flagged = {name: int(tr.graph(c["idx"], c["dist"], c["Y"])["flagged"].sum()) for name, c in tr.list_cases().items()}
    assert not any(flagged.values()), "a list case comes too close to a threshold: choose another seed (%s)" % flagged

    X, grp = ur.blobs()
    ref, tgt = tr.held_out()
    Xr, Z = np.ascontiguousarray(X[ref]), np.ascontiguousarray(X[tgt])
    a, b = _umap.find_ab_params(1.0, 0.1)
    ref_Y, share, same_group, start_share = [], np.zeros((len(DIMS), len(SEEDS))), np.zeros((len(DIMS), len(SEEDS)), dtype=bool), []
    whole_y = None
    for di, dims in enumerate(DIMS):
        Y = ur.run(Xr, REF_K, dims, REF_EPOCHS, a, b, REF_SEED, _umap.start_positions("pca", Xr, len(Xr), dims, REF_SEED), fit_group)
        ref_Y.append(Y)
        for seed in SEEDS:
            y0, y = tr.run(Z, Xr, Y, WHOLE_K, WHOLE_EPOCHS, a, b, seed, group)
            s, ie = tr.target_share(y, Y, Z, Xr)
            share[di, seed] = s
            same_group[di, seed] = bool((grp[ref][ie] == grp[tgt][:, None]).all())
            if dims == 2 and seed == 0:
                whole_y = y
        start_share.append(tr.target_share(y0, Y, Z, Xr)[0])
        print("%d dimensions: share %.4f .. %.4f (the start alone %.4f), groups kept: %s"
              % (dims, share[di].min(), share[di].max(), start_share[-1], same_group[di].all()), flush=True)
    np.savez(args.out, ref_rows=ref, target_rows=tgt, ref_Y2=ref_Y[0], ref_Y3=ref_Y[1], dims=np.array(DIMS, dtype=np.int64),
             seeds=np.array(SEEDS, dtype=np.int64), whole_k=np.int64(WHOLE_K), whole_epochs=np.int64(WHOLE_EPOCHS), share=share,
             same_group=same_group, start_share=np.array(start_share), whole_y_seed0_dims2=whole_y,
             list_flagged=np.int64(sum(flagged.values())), group=np.int64(group), ab=np.array([a, b]),
             written=np.array(datetime.date.today().isoformat()))
    print("-> %s" % args.out)


if __name__ == "__main__":
    main()
