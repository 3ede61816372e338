"""The two-level stream's mode control by reference bucket (nabo_amd/csrc/l2c_topk.hip): a wave keeps one refetch account per
bucket of the references, walks the table of bucket ends (nabo_amd/csrc/local_seeds.h: lseed_bucket_ends) in its refetch path
and runs the two-step loop to the end of a bucket whose account is spent.  The control decides only WHICH loop runs a tile,
never what is computed: every row must be the oracle's bits, under the new control and under the one before it
("two_level_stretch" = 16), on the setup of tests/test_two_level_gpu.py -- 700 rows x 5000 references, d = 50, k = 15.

"local_anchors" = 64 makes most buckets 2 - 3 tiles long: ends on odd tile indices, buckets shorter than the loop's step of
two.  A mask over one far cluster that holds an anchor cell empties that anchor's bucket: two equal consecutive ends.

The counter bound follows from the rule: per wave and bucket of T_b tiles the account pays burst + share T_b / 100 refetches
and the pair of tiles in flight when it is spent may add one -- summed, with sum T_b <= the stream's tiles,
refetched <= W (C (burst + 1) + share x tiles / 100) for W waves that ran."""
import functools

import numpy as np
import pytest

import oracle
from nabo_amd._synth import pca_like

pytestmark = pytest.mark.gpu

M, N, K, G = 700, 5000, 15, 50
BURST, SHARE = 3, 25                      # the control's defaults (l2c_topk.hip)
KEYS = ("two_level_one_step_tiles", "two_level_refetched_tiles", "two_level_two_step_tiles")


def _opts(anchors, **more):
    return dict({"two_level": 2, "splits": 1, "local_anchors": anchors}, **more)


@functools.lru_cache(maxsize=None)
def _data(kind):
    """(X, Y, mask, the oracle's answer), computed once per kind and left unchanged"""
    mask = None
    if kind == "cloud":
        rng = np.random.default_rng(5)
        Y, X = rng.standard_normal((N, G)), rng.standard_normal((M, G))
    elif kind == "lattice":
        rng = np.random.default_rng(7)
        L = rng.integers(0, 3, (N - 500, G)).astype(np.float64)
        Y = np.concatenate([L, L[:500]])
        X = np.concatenate([L[100:100 + M // 2], rng.integers(0, 3, (M - M // 2, G)).astype(np.float64)])
    else:
        Y, X = pca_like(N, G, seed=11), pca_like(M, G, seed=12)
        if kind == "masked":
            # anchor 2 of 4 is reference cell 2 * (N // 4): it and its 100 neighbours in the array form a cluster of their
            # own, far from all other cells, and all of it is masked -- no unmasked cell is nearest to that anchor
            a = 2 * (N // 4)
            Y = Y.copy()
            Y[a - 50:a + 51] = 60.0 + np.random.default_rng(13).standard_normal((101, G))
            mask = np.zeros(N, dtype=np.uint8)
            mask[::3] = 1
            mask[a - 50:a + 51] = 1
    oi, od = oracle.knn(X, Y, K, 0, ref_mask=mask, nthreads=8)
    for a in (X, Y, oi, od):
        a.setflags(write=False)
    return X, Y, mask, oi, od


def _run(gpu_lib, kind, opts):
    X, Y, mask, oi, od = _data(kind)
    ix = gpu_lib.KnnIndex(N, G, options=opts).set_ref(Y, ref_mask=mask)
    gi, gd = ix.query(X, K)
    st, kern = ix.last_stats(), ix.last_kernel()
    ix.close()
    assert np.array_equal(gi, oi) and np.array_equal(gd, od), int((gi != oi).any(axis=1).sum())
    assert kern.startswith("l2c_topk_kernel<2,1,23,6,32,4,2>") and "two-level tiles" in kern, kern
    c = tuple(int(st[a]) for a in KEYS)
    print(kind, opts, c)
    return c


def _both(gpu_lib, kind, anchors, **more):
    """the per-bucket control and the one before it: the same bits (checked in _run), every tile run by one loop or the other
    in both, and the bound on the refetches that follows from the per-bucket rule"""
    new = _run(gpu_lib, kind, _opts(anchors, **more))
    old = _run(gpu_lib, kind, _opts(anchors, two_level_stretch=16, **more))
    assert new[0] + new[2] == old[0] + old[2] > 0, (new, old)
    tiles = (-(-N // 32) + anchors + 1) // 2 * 2          # lseed_ordered_tiles: what every wave that ran streams
    assert (new[0] + new[2]) % tiles == 0, (new, tiles)
    waves = (new[0] + new[2]) // tiles
    burst, share = more.get("two_level_burst", BURST), more.get("two_level_share", SHARE)
    assert new[1] * 100 <= waves * (anchors * (burst + 1) * 100 + share * tiles), (new, waves, tiles)
    return new, old


@pytest.mark.parametrize("anchors", [4, 16, 64])
def test_clustered_data_by_bucket_and_by_stretch(gpu_lib, anchors):
    new, old = _both(gpu_lib, "pca", anchors)
    assert new[0] > 0 and new != old, (new, old)           # clustered data: the two controls cut the stream differently


def test_a_spent_account_runs_two_step_to_the_buckets_end(gpu_lib):
    """burst 1 and the smallest share: the first refetch of a bucket sends the wave two-step to its end"""
    new, _ = _both(gpu_lib, "pca", 16, two_level_burst=1, two_level_share=1)
    assert new[2] > 0 and new[0] > 0, new


def test_a_masked_third_and_an_empty_bucket(gpu_lib):
    _both(gpu_lib, "masked", 4)


def test_one_gaussian_cloud_every_bucket_dense(gpu_lib):
    new, _ = _both(gpu_lib, "cloud", 4)
    assert new[2] > new[0] > 0, new                        # each bucket's first tiles one-step, the rest of it two-step


def test_a_lattice_with_exact_ties(gpu_lib):
    _both(gpu_lib, "lattice", 4)
    _both(gpu_lib, "lattice", 64)
