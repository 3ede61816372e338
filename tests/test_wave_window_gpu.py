"""The progress window of a workgroup in the two-level stream's main launch (nabo_amd/csrc/l2c_window.h, l2c_topk.hip): a wave
that runs more than "two_level_window" tiles ahead of the slowest live wave of its workgroup sleeps.  That changes when a
wave runs and nothing else, so with no window (-1), the default (0), the narrowest (1, looking at every pair of tiles) and
the clamp's maximum, indices, the bits of the distances and the three tile counters are the same, and the oracle's.

On the setup of tests/test_two_level_gpu.py (700 rows x 5000 references, d = 50, k = 15, "two_level" = 2, four buckets).  The
padding cases use four Gaussian clusters laid out so that the buckets are known without a GPU: the anchors are the
reference cells 0, N/4, 2N/4, 3N/4 (local_seeds.hip), one per cluster, every row is several times nearer to its own
cluster's anchor than to any other (asserted), so a row's bucket is its cluster.  From the rows per bucket the layout rules
of local_seeds.h give the positions of the bucket-ordered copy, 96 of them per wave and 384 per workgroup: which waves are
all padding -- they leave at once, beside live ones that must not wait for them -- is computed here and asserted."""
import functools

import numpy as np
import pytest

import oracle
from nabo_amd import _knn
from nabo_amd._synth import pca_like

pytestmark = pytest.mark.gpu

TL = {"two_level": 2, "splits": 1, "local_anchors": 4}
M, N, K, G, C = 700, 5000, 15, 50, 4
COL_ROWS, WAVE_ROWS, WG_WAVES = 128, 96, 4                       # local_seeds.h: LSEED_COL_ROWS; geometry B of l2c_topk.hip
WINDOWS = ({"two_level_window": -1}, {}, {"two_level_window": 1, "two_level_check": 2},
           {"two_level_window": 10 ** 6, "two_level_check": 10 ** 6})            # none, the default, narrowest, the clamps
COUNTERS = ("two_level_one_step_tiles", "two_level_refetched_tiles", "two_level_two_step_tiles")


@functools.lru_cache(maxsize=None)
def _pca():
    Y, X = pca_like(N, G, seed=11), pca_like(M, G, seed=12)
    oi, od = oracle.knn(X, Y, K, 0, nthreads=8)
    for a in (X, Y, oi, od):
        a.setflags(write=False)
    return X, Y, oi, od


@functools.lru_cache(maxsize=None)
def _clusters():
    """references: cluster c is the cells [c N/4, (c + 1) N/4); rows: 700 with random clusters, then 96 of cluster 3"""
    rng = np.random.default_rng(31)
    centres = 20.0 * np.eye(C, G)
    Y = np.repeat(centres, N // C, axis=0) + rng.standard_normal((N, G))
    lab = np.concatenate([rng.integers(0, C, M), np.full(WAVE_ROWS, 3)])
    X = centres[lab] + rng.standard_normal((len(lab), G))
    d2 = ((X[:, None, :] - Y[None, ::N // C, :]) ** 2).sum(axis=2)              # to the four anchor cells
    assert (d2.argmin(axis=1) == lab).all() and (np.sort(d2, axis=1)[:, 1] > 2.0 * d2.min(axis=1)).all()
    for a in (X, Y, lab):
        a.setflags(write=False)
    return X, Y, lab


@functools.lru_cache(maxsize=None)
def _cluster_oracle(lo, hi):
    X, Y, _ = _clusters()
    oi, od = oracle.knn(X[lo:hi], Y, K, 0, nthreads=8)
    oi.setflags(write=False)
    od.setflags(write=False)
    return oi, od


def _live_waves(row_cnt, ref_cnt, lkeep):
    """local_seeds.h on the host: lseed_tournament / lseed_layout (query side) / lseed_columns -> per workgroup of the
    ordered main launch, which of its four waves hold a row at all"""
    q = (lkeep + 3) // 4
    has_t = [-(-int(r) // 32) >= 6 * q for r in ref_cnt]                        # lseed_tournament: pt != 0
    live, pos = [], 0
    for b in range(C):
        if has_t[b]:
            live += list(range(pos, pos + int(row_cnt[b])))
            pos += -(-int(row_cnt[b]) // COL_ROWS) * COL_ROWS
    rest = sum(int(row_cnt[b]) for b in range(C) if not has_t[b])               # the rest class, back to back
    live += list(range(pos, pos + rest))
    rows = int(sum(row_cnt))
    prow = (-(-rows // COL_ROWS) + C + 1) * COL_ROWS                            # lseed_columns x LSEED_COL_ROWS
    nwg = -(-prow // (WAVE_ROWS * WG_WAVES))
    w = np.zeros(nwg * WG_WAVES, dtype=bool)
    w[np.unique(np.asarray(live) // WAVE_ROWS)] = True
    return w.reshape(nwg, WG_WAVES)


def _query(gpu_lib, X, Y, more):
    ix = gpu_lib.KnnIndex(Y.shape[0], Y.shape[1], options=dict(TL, **more)).set_ref(Y)
    gi, gd = ix.query(X, K)
    st, kern = ix.last_stats(), ix.last_kernel()
    ix.close()
    assert kern.startswith("l2c_topk_kernel<2,1,23,6,32,4,2>") and "two-level tiles" in kern, kern
    return gi, gd, tuple(st[c] for c in COUNTERS)


def _all_windows(gpu_lib, X, Y, oi, od):
    got = [_query(gpu_lib, X, Y, w) for w in WINDOWS]
    print([g[2] for g in got])
    for gi, gd, cnt in got:
        assert np.array_equal(gi, oi) and gd.dtype == od.dtype and gd.tobytes() == od.tobytes()
        assert cnt == got[0][2] and cnt[0] + cnt[2] > 0, (cnt, got[0][2])
    return got[0][2]


def test_the_options_exist_and_are_clamped(gpu_lib):
    ix = gpu_lib.KnnIndex(N, G, options=dict(TL, two_level_window=-5, two_level_check=-5))
    ix.close()
    assert _knn.query_plan(N, G, M, K, options=dict(TL, two_level_window=1, two_level_check=2))["two_level"] == 2


def test_every_window_gives_the_same_bits_and_tile_counters(gpu_lib):
    X, Y, oi, od = _pca()
    cnt = _all_windows(gpu_lib, X, Y, oi, od)
    assert cnt[0] > 0 and cnt[1] > 0, cnt                # both loops' checks ran: one-step tiles, refetches among them


def test_one_broad_cloud_runs_the_window_in_the_two_step_loop(gpu_lib):
    rng = np.random.default_rng(5)
    Y, X = rng.standard_normal((N, G)), rng.standard_normal((M, G))
    oi, od = oracle.knn(X, Y, K, 0, nthreads=8)
    cnt = _all_windows(gpu_lib, X, Y, oi, od)
    assert cnt[2] > cnt[0] > 0, cnt


@pytest.mark.parametrize("lo,hi,one_live", [(0, 1, True), (0, 97, True), (0, 385, True), (M, M + WAVE_ROWS, True)])
def test_all_padding_waves_beside_live_ones(gpu_lib, lo, hi, one_live):
    """1, 97 and 385 rows of random clusters, and 96 rows of ONE cluster: a single full wave, its three partners all padding"""
    X, Y, lab = _clusters()
    lkeep = _knn.query_plan(N, G, hi - lo, K, options=TL)["lkeep"]
    ref_cnt = [N // C] * C
    live = _live_waves(np.bincount(lab[lo:hi], minlength=C), ref_cnt, lkeep)
    per_wg = live.sum(axis=1)
    assert ((per_wg > 0) & (per_wg < WG_WAVES)).any(), live               # a workgroup with dead waves beside live ones
    assert (per_wg == 1).any() == one_live, live                          # ... and one with exactly one live wave
    if hi - lo == WAVE_ROWS:
        assert live[0].tolist() == [True, False, False, False] and not live[1:].any(), live
    oi, od = _cluster_oracle(lo, hi)
    _all_windows(gpu_lib, X[lo:hi], Y, oi, od)
