"""Local tournament seeds (nabo_amd/csrc/local_seeds.hip): the one-split launches of the one-product pass start every
row's list from a tournament over the row's own bucket of the references instead of the stream's first tiles.  A seed only
decides where a list STARTS, so every result must be the oracle's bits with the option on and off; a seed that is too
low would show as rows the first pass no longer answers (nabo_index_last_passes).

The shapes are the smallest that reach the path: option "splits" = 1 keeps a few hundred rows in one reference split,
"local_seeds" = 2 takes local seeds below the sizes the planner would, "local_anchors" picks few enough buckets that a
bucket of a few thousand references is long enough for a tournament (6 ceil(lkeep / 4) tiles)."""
import functools

import numpy as np
import pytest

import oracle
from nabo_amd import _knn, _sharded
from nabo_amd._synth import pca_like

pytestmark = pytest.mark.gpu

ON = {"splits": 1, "local_seeds": 2, "local_anchors": 4}
OFF = {"splits": 1, "local_seeds": 0}


@functools.lru_cache(maxsize=None)
def _data(n, g, m, seed):
    Y, X = pca_like(n, g, seed=seed), pca_like(m, g, seed=seed + 1)
    Y.setflags(write=False)
    X.setflags(write=False)
    return X, Y


@functools.lru_cache(maxsize=None)
def _oracle(n, g, m, seed, k, metric):
    X, Y = _data(n, g, m, seed)
    return oracle.knn(X, Y, k, metric, nthreads=8)


def _query(gpu_lib, X, Y, k, opts, metric=0, mask=None, base=0, drop=False):
    ix = gpu_lib.KnnIndex(Y.shape[0], Y.shape[1], metric=metric, ref_index_base=base, options=opts).set_ref(Y, ref_mask=mask)
    gi, gd = ix.query(X, k, drop_first=drop)
    out = (gi, gd, ix.last_stats(), ix.last_row_pass(X.shape[0]), ix.last_kernel())
    ix.close()
    return out


def _both(gpu_lib, X, Y, k, oi, od, on=ON, off=OFF, **kw):
    """on and off against the oracle; the first pass answers no fewer rows with local seeds than without"""
    res = {}
    for name, opts in (("on", on), ("off", off)):
        gi, gd, st, rp, kern = _query(gpu_lib, X, Y, k, opts, **kw)
        assert np.array_equal(gi, oi) and np.array_equal(gd, od), (name, int((gi != oi).any(axis=1).sum()))
        assert st["splits"] == 1 and "l2c_topk_kernel" in kern, (st, kern)
        res[name] = (st, rp, kern)
    assert int((res["on"][1] == 0).sum()) >= int((res["off"][1] == 0).sum())
    return res


@pytest.mark.parametrize("g", [50, 7])
def test_300_targets_5000_references(gpu_lib, g):
    X, Y = _data(5000, g, 300, 11)
    oi, od = _oracle(5000, g, 300, 11, 15, 0)
    assert _knn.query_plan(5000, g, 300, 15, options=ON)["local_seed_buckets"] == 4
    _both(gpu_lib, X, Y, 15, oi, od)


def test_references_no_multiple_of_a_tile_and_one_target_row(gpu_lib):
    X, Y = _data(5000, 50, 300, 11)
    Yo = Y[:4983]
    oi, od = oracle.knn(X, Yo, 15, 0, nthreads=8)
    _both(gpu_lib, X, Yo, 15, oi, od)
    _both(gpu_lib, X[7:8], Yo, 15, oi[7:8], od[7:8])


def test_all_references_in_one_bucket_and_a_bucket_beyond_its_cap(gpu_lib):
    """Duplicated anchor cells: every anchor is the same point, ties go to the lowest anchor, bucket 0 holds everything --
    and with local_cap = 2048 only its first 2048 cells."""
    X, Y = _data(5000, 50, 300, 11)
    Yd = Y.copy()
    Yd[1250::1250][:3] = Yd[0]                               # the anchors are the cells 0, 1250, 2500, 3750
    oi, od = oracle.knn(X, Yd, 15, 0, nthreads=8)
    _both(gpu_lib, X, Yd, 15, oi, od)
    _both(gpu_lib, X, Yd, 15, oi, od, on=dict(ON, local_cap=2048))


def test_buckets_too_small_for_a_tournament_leave_every_row_to_the_rest_class(gpu_lib):
    """256 buckets of ~20 references: none reaches the 36 tiles a tournament for 23-entry lists needs, every row keeps the
    stream-prefix tournament -- and so exactly the rows of the run without local seeds go on to the seeded pass."""
    X, Y = _data(5000, 50, 300, 11)
    oi, od = _oracle(5000, 50, 300, 11, 15, 0)
    res = _both(gpu_lib, X, Y, 15, oi, od, on=dict(ON, local_anchors=256))
    assert np.array_equal(res["on"][1], res["off"][1])


def test_masked_nearest_references_and_set_mask_after_set_ref(gpu_lib):
    """The targets are references; mask exactly those: a masked cell in a bucket's run would seed every such row with 0."""
    _, Y = _data(5000, 50, 300, 11)
    X = Y[:600:2] + 1e-9
    mask = np.zeros(5000, dtype=np.uint8)
    mask[:600:2] = 1
    mask[3000:3400] = 1
    oi, od = oracle.knn(X, Y, 15, 0, ref_mask=mask, nthreads=8)
    _both(gpu_lib, X, Y, 15, oi, od, mask=mask)
    o0i, o0d = oracle.knn(X, Y, 15, 0, nthreads=8)
    ix = gpu_lib.KnnIndex(5000, 50, options=ON).set_ref(Y)
    gi, gd = ix.query(X, 15)
    assert np.array_equal(gi, o0i) and np.array_equal(gd, o0d)
    ix.set_mask(mask)                                        # the runs are rebuilt from the repacked operands
    gi, gd = ix.query(X, 15)
    assert np.array_equal(gi, oi) and np.array_equal(gd, od)
    ix.set_mask(None)
    gi, gd = ix.query(X, 15)
    ix.close()
    assert np.array_equal(gi, o0i) and np.array_equal(gd, o0d)


def test_geometry_a_and_geometry_c(gpu_lib):
    """28 kept entries on the 32-entry lists (geometry A, pinned), and cosine d = 100, k = 50 on the 64-entry lists
    (geometry C: 16 values per lane, 96-tile tournaments, so two buckets of ~4000)."""
    X, Y = _data(8000, 50, 300, 21)
    oi, od = _oracle(8000, 50, 300, 21, 20, 0)
    res = _both(gpu_lib, X, Y, 20, oi, od, on=dict(ON, l2c_geo=0), off=dict(OFF, l2c_geo=0))
    assert "1,33,8,64,4,1" in res["on"][2]
    X, Y = _data(8000, 100, 300, 31)
    oi, od = _oracle(8000, 100, 300, 31, 50, 2)
    res = _both(gpu_lib, X, Y, 50, oi, od, on=dict(ON, local_anchors=2), metric=2)
    assert "2,65,4,64,4,1" in res["on"][2]


def test_reference_index_base_and_self_drop(gpu_lib):
    X, Y = _data(5000, 50, 300, 11)
    oi, od = _oracle(5000, 50, 300, 11, 15, 0)
    _both(gpu_lib, X, Y, 15, oi + 1000, od, base=1000)
    si, sd = oracle.knn(Y[:300], Y, 15, 0, drop_first=True, nthreads=8)
    _both(gpu_lib, Y[:300], Y, 15, si, sd, drop=True)


def test_two_loopback_shard_ranks(gpu_lib):
    X, Y = _data(10000, 50, 300, 41)
    oi, od = _oracle(10000, 50, 300, 41, 15, 0)
    for opts in (ON, OFF):
        grp = _sharded.ShardedGroup([0, 0], 10000, 50, 0, Y, transport="loopback")
        for ix in grp.indices:
            for name, value in opts.items():
                ix.set_option(name, value)
        grp.set_ref()
        gi, gd = grp.query(X, 15)
        grp.close()
        assert np.array_equal(gi, oi) and np.array_equal(gd, od)


def test_the_first_pass_answers_no_fewer_rows_with_local_seeds(gpu_lib):
    """2000 rows over 20000 references in 8 buckets, lists of k + 2 kept entries so that the first pass cannot certify a
    good part of the rows either way: a list that starts lower ends as the same lkeep smallest scores, so the rows that
    go on to the seeded pass (nabo_index_last_passes through last_stats) are no more than without local seeds."""
    X, Y = _data(20000, 50, 2000, 51)
    oi, od = _oracle(20000, 50, 2000, 51, 15, 0)
    res = _both(gpu_lib, X, Y, 15, oi, od, on=dict(ON, local_anchors=8, lkeep=17), off=dict(OFF, lkeep=17))
    on, off = res["on"][0], res["off"][0]
    print("rows to the seeded pass: local seeds %d, stream prefix %d" % (on["seeded_pass_rows"], off["seeded_pass_rows"]))
    assert off["seeded_pass_rows"] > 0, "the case has no teeth: every row certified by the first pass"
    assert on["seeded_pass_rows"] <= off["seeded_pass_rows"]
