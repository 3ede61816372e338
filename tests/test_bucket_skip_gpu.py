"""The two-level stream skips the sub-buckets a workgroup's rows cannot reach (nabo_amd/csrc/bucket_skip.h, bucket_skip.hip;
option "bucket_skip").  The skip drops a stretch of the reference stream on a rigorous lower bound of the distances, so it
decides only WHICH tiles a workgroup runs, never what is found: every row must be the oracle's bits, with the skip forced on
("bucket_skip" = 2), switched off (1) and left at its default under a forced stream (no skip), on the setup of
tests/test_bucket_mode_gpu.py -- 700 rows x 5000 references, d = 50, k = 15 -- with 4, 16 and 64 anchors.

Every tile of the stream is accounted for exactly once per wave that ran: one-step + two-step + skipped is a whole multiple of
the stream's tiles."""
import functools

import numpy as np
import pytest

import oracle
from nabo_amd._synth import pca_like

pytestmark = pytest.mark.gpu

M, N, K = 700, 5000, 15
KEYS = ("two_level_one_step_tiles", "two_level_refetched_tiles", "two_level_two_step_tiles", "two_level_skipped_tiles")
ANCHORS = (4, 16, 64)


def _opts(anchors, **more):
    return dict({"two_level": 2, "splits": 1, "local_anchors": anchors, "bucket_skip": 2}, **more)


@functools.lru_cache(maxsize=None)
def _data(kind):
    """(X, Y, mask, the oracle's answer), computed once per kind and left unchanged"""
    mask, g = None, 50
    if kind == "clusters":
        # four tight clusters of 1250 cells, 20 widths from each other (tests/test_two_level_gpu.py)
        rng = np.random.default_rng(17)
        centres = 20.0 * np.eye(4, g)
        Y = centres[np.repeat([0, 1, 2, 3], N // 4)] + rng.standard_normal((N, g))
        X = centres[rng.integers(0, 4, M)] + rng.standard_normal((M, g))
    elif kind == "cloud":
        rng = np.random.default_rng(5)
        Y, X = rng.standard_normal((N, g)), rng.standard_normal((M, g))
    elif kind == "lattice":
        rng = np.random.default_rng(7)
        L = rng.integers(0, 3, (N - 500, g)).astype(np.float64)
        Y = np.concatenate([L, L[:500]])
        X = np.concatenate([L[100:100 + M // 2], rng.integers(0, 3, (M - M // 2, g)).astype(np.float64)])
    elif kind == "far":
        # clusters of unit width 800 widths from the centre of the data: rows go down the pass chain
        rng = np.random.default_rng(6)
        centres = rng.standard_normal((8, g))
        centres *= 800.0 / np.linalg.norm(centres, axis=1, keepdims=True)
        Y = centres[rng.integers(0, 8, N)] + rng.standard_normal((N, g))
        X = centres[rng.integers(0, 8, M)] + rng.standard_normal((M, g))
    elif kind in ("d29", "d59"):
        g = int(kind[1:])
        Y, X = pca_like(N, g, seed=21), pca_like(M, g, seed=22)
    else:
        Y = pca_like(N, g, seed=11)
        X = pca_like(1100 if kind == "m1100" else M, g, seed=12)
        if kind == "one_row":
            X = X[5:6]
        if kind == "masked":
            # anchor 2 of 4 is reference cell 2 * (N // 4): it and its 100 neighbours in the array form a cluster of their
            # own, far from all other cells, and all of it is masked -- no unmasked cell is nearest to that anchor
            a = 2 * (N // 4)
            Y = Y.copy()
            Y[a - 50:a + 51] = 60.0 + np.random.default_rng(13).standard_normal((101, g))
            mask = np.zeros(N, dtype=np.uint8)
            mask[::3] = 1
            mask[a - 50:a + 51] = 1
    oi, od = oracle.knn(X, Y, K, 0, ref_mask=mask, nthreads=8)
    for a in (X, Y, oi, od):
        a.setflags(write=False)
    return X, Y, mask, oi, od


def _run(gpu_lib, kind, opts):
    X, Y, mask, oi, od = _data(kind)
    ix = gpu_lib.KnnIndex(N, Y.shape[1], options=opts).set_ref(Y, ref_mask=mask)
    gi, gd = ix.query(X, K)
    st, kern = ix.last_stats(), ix.last_kernel()
    ix.close()
    c = tuple(int(st[a]) for a in KEYS)
    print(kind, opts, c)
    assert np.array_equal(gi, oi) and np.array_equal(gd, od), int((gi != oi).any(axis=1).sum())
    assert kern.startswith("l2c_topk_kernel<2,1,23,6,32,4,2>") and "two-level tiles" in kern, kern
    tiles = (-(-N // 32) + opts["local_anchors"] + 1) // 2 * 2          # lseed_ordered_tiles: what every wave that ran accounts for
    assert c[0] + c[2] + c[3] > 0 and (c[0] + c[2] + c[3]) % tiles == 0, (c, tiles)
    return c


@pytest.mark.parametrize("anchors", ANCHORS)
def test_well_separated_clusters_skip_tiles(gpu_lib, anchors):
    c = _run(gpu_lib, "clusters", _opts(anchors))
    assert c[3] > 0, c


@pytest.mark.parametrize("anchors", ANCHORS)
@pytest.mark.parametrize("kind", ["pca", "cloud", "lattice", "masked", "far", "one_row", "m1100", "d29", "d59"])
def test_the_oracles_bits_whatever_is_skipped(gpu_lib, kind, anchors):
    c = _run(gpu_lib, kind, _opts(anchors))
    if kind in ("pca", "masked", "m1100", "d29", "d59"):
        assert c[3] > 0, c          # clustered kinds: the rule does skip at every anchor count, so the bits above test it


@pytest.mark.parametrize("anchors", ANCHORS)
@pytest.mark.parametrize("kind", ["clusters", "pca", "masked"])
def test_switched_off_and_by_default_nothing_is_skipped(gpu_lib, kind, anchors):
    on = _run(gpu_lib, kind, _opts(anchors))
    off = _run(gpu_lib, kind, _opts(anchors, bucket_skip=1))
    dflt = _run(gpu_lib, kind, {"two_level": 2, "splits": 1, "local_anchors": anchors})
    assert off[3] == 0 and dflt[3] == 0, (off, dflt)
    assert off == dflt and on[0] + on[2] + on[3] == off[0] + off[2], (on, off, dflt)
