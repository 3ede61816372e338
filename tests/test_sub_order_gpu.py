"""The sub-order inside the buckets of the two-level stream (nabo_amd/csrc/local_seeds.h, options "two_level_sub" and
"two_level_sub_rank"): both bucket-ordered copies sort a bucket's cells by their nearest of S sub-anchors.  An order of the
stream decides which tiles pass the first step's bound and nothing else, so with S = 1 (off), 2, 8 and the clamp's maximum
(64) every query must return the oracle's indices and the bits of its distances -- all rows are compared.

Every query must also have run the stream (its tile counters moved), and the maps of the two copies
(nabo_index_stream_order) must hold every row and every unmasked reference exactly once, at the positions the buckets
had with S = 1: only the places inside a bucket move."""
import functools

import numpy as np
import pytest

import oracle
from nabo_amd import _knn
from nabo_amd._synth import pca_like

pytestmark = pytest.mark.gpu

TL = {"two_level": 2, "splits": 1, "local_anchors": 4}
SUBS = (1, 2, 8, 10 ** 6)                 # off, the smallest, a usual one, the clamp (64)
G, K = 50, 15
NONE = 0xFFFFFFFF
RAN = "two-level tiles"


@functools.lru_cache(maxsize=None)
def _pca(n, m, seed, g=G):
    Y, X = pca_like(n, g, seed=seed), pca_like(m, g, seed=seed + 1)
    Y.setflags(write=False)
    X.setflags(write=False)
    return X, Y


@functools.lru_cache(maxsize=None)
def _big():
    X, Y = _pca(20000, 20000, 51)
    oi, od = oracle.knn(X, Y, K, 0, nthreads=16)
    oi.setflags(write=False)
    od.setflags(write=False)
    return X, Y, oi, od


def _check(ix, X, want, m, live, what, k=K, drop=False):
    """one query against the oracle's bits; the stream ran; both maps hold every row / live reference once"""
    gi, gd = ix.query(X, k, drop_first=drop)
    st, kern = ix.last_stats(), ix.last_kernel()
    oi, od = want
    assert np.array_equal(gi, oi) and gd.dtype == od.dtype and gd.tobytes() == od.tobytes(), (what, int((gi != oi).any(axis=1).sum()))
    assert RAN in kern and st["two_level_one_step_tiles"] + st["two_level_two_step_tiles"] > 0, (what, kern)
    rows, refs = ix.stream_order()
    assert np.array_equal(np.sort(rows[rows != NONE]), np.arange(m)), what
    assert np.array_equal(np.sort(refs[refs != NONE]), live), what
    return st, rows, refs


def _sweep(gpu_lib, X, Y, what, metric=0, mask=None, opts=TL, drop=False, want=None, expect_moved=True, k=K):
    """the same query at every S of SUBS; returns the maps per S"""
    n = Y.shape[0]
    if want is None:
        want = oracle.knn(X, Y, k, metric, ref_mask=mask, drop_first=drop, nthreads=16)
    live = np.flatnonzero(mask == 0) if mask is not None else np.arange(n)
    out = {}
    for s in SUBS:
        o = dict(opts, two_level_sub=s)
        assert _knn.query_plan(n, Y.shape[1], X.shape[0], k, metric=metric, drop_first=drop, options=o)["two_level"] == 2, (what, s)
        ix = gpu_lib.KnnIndex(n, Y.shape[1], metric=metric, options=o).set_ref(Y, ref_mask=mask)
        try:
            st, rows, refs = _check(ix, X, want, X.shape[0], live, "%s, S = %d" % (what, s), k=k, drop=drop)
        finally:
            ix.close()
        print(what, "S =", s, {a: b for a, b in st.items() if a.startswith("two_level") or a == "seeded_pass_rows"})
        out[s] = (rows, refs)
    for s in SUBS[1:]:                                       # the buckets stay where they were: padding at the same positions
        for a, b in zip(out[s], out[1]):
            assert np.array_equal(a == NONE, b == NONE), (what, s)
    if expect_moved:
        assert any(not np.array_equal(out[s][1], out[1][1]) for s in SUBS[1:]), "%s: no reference moved at any S" % what
    return out


def test_as_many_anchors_as_references(gpu_lib):
    """64 references, 64 buckets of one cell: fewer cells than any S, nothing may move"""
    X, Y = _pca(64, 124, 3)
    out = _sweep(gpu_lib, X, Y, "n = anchors = 64", opts=dict(TL, local_anchors=64), expect_moved=False)
    for s in SUBS[1:]:
        assert np.array_equal(out[s][0], out[1][0]) and np.array_equal(out[s][1], out[1][1])


def test_a_bucket_with_fewer_cells_than_sub_anchors(gpu_lib):
    """four tight clusters, the anchors (cells 0, 1250, 2500, 3750) one in each; the last cluster has five cells: sorted by
    two sub-anchors, left in caller order by eight"""
    rng = np.random.default_rng(17)
    n, m = 5000, 700
    lab = np.repeat([0, 1, 2], [1250, 1250, 2500])
    lab[3750:3755] = 3
    centres = 20.0 * np.eye(4, G)
    Y = centres[lab] + rng.standard_normal((n, G))
    X = centres[rng.integers(0, 4, m)] + rng.standard_normal((m, G))
    out = _sweep(gpu_lib, X, Y, "a bucket of five cells")
    tiny = np.arange(3750, 3755)
    for s in SUBS:
        refs = out[s][1]
        at = np.flatnonzero(np.isin(refs, tiny))
        assert len(at) == 5 and at[-1] - at[0] == 4, (s, at)                   # the bucket's five positions
        if s != 2:
            assert np.array_equal(refs[at], tiny), (s, refs[at])                # S = 1, 8, 64: caller order


def test_a_padded_last_tile(gpu_lib):
    X, Y = _pca(4097, 385, 5, g=59)
    _sweep(gpu_lib, X, Y, "n = 4097, d = 59")


@pytest.mark.parametrize("s", SUBS)
def test_twenty_thousand_clustered_cells_with_the_default_buckets(gpu_lib, s):
    X, Y, oi, od = _big()
    o = {"two_level": 2, "splits": 1, "two_level_sub": s}
    assert _knn.query_plan(20000, G, 20000, K, options=o)["two_level"] == 2
    ix = gpu_lib.KnnIndex(20000, G, options=o).set_ref(Y)
    try:
        st, _, _ = _check(ix, X, (oi, od), 20000, np.arange(20000), "20000 x 20000, S = %d" % s)
    finally:
        ix.close()
    print("S =", s, {a: b for a, b in st.items() if a.startswith("two_level") or a == "seeded_pass_rows"})


def test_a_mask_that_hides_a_sub_anchor(gpu_lib):
    """the second of bucket 0's eight sub-anchors, found from the order with S = 1, is masked (and an anchor cell with it):
    the bucket draws other sub-anchors, the hidden cell is in no copy"""
    X, Y = _pca(5000, 700, 11)
    ix = gpu_lib.KnnIndex(5000, G, options=dict(TL, two_level_sub=1)).set_ref(Y)
    try:
        ix.query(X, K)
        _, refs = ix.stream_order()
    finally:
        ix.close()
    first = refs[:int(np.flatnonzero(refs == NONE)[0])]                         # bucket 0, caller order
    assert len(first) >= 64
    mask = np.zeros(5000, dtype=np.uint8)
    mask[first[len(first) // 8]] = 1
    mask[1250] = 1
    mask[::7] = 1
    _sweep(gpu_lib, X, Y, "a masked sub-anchor", mask=mask)


def test_one_resident_index_through_set_ref_set_mask_and_other_s(gpu_lib):
    X1, Y1 = _pca(5000, 700, 11)
    X2, Y2 = _pca(5000, 300, 31)
    mask = np.zeros(5000, dtype=np.uint8)
    mask[::3] = 1
    all_refs = np.arange(5000)
    ix = gpu_lib.KnnIndex(5000, G, options=dict(TL, two_level_sub=8))
    try:
        ix.set_ref(Y1)
        _, _, r8 = _check(ix, X1, oracle.knn(X1, Y1, K, 0, nthreads=16), 700, all_refs, "set_ref(Y1), S = 8")
        ix.set_option("two_level_sub", 2)
        ix.set_ref(Y2)
        _check(ix, X2, oracle.knn(X2, Y2, K, 0, nthreads=16), 300, all_refs, "S = 2, then set_ref(Y2)")
        ix.set_option("two_level_sub", 8)
        ix.set_mask(mask)
        _check(ix, X2, oracle.knn(X2, Y2, K, 0, ref_mask=mask, nthreads=16), 300, np.flatnonzero(mask == 0), "S = 8, set_mask")
        ix.set_mask(None)
        ix.set_option("two_level_sub", 1)
        _, _, r1 = _check(ix, X2, oracle.knn(X2, Y2, K, 0, nthreads=16), 300, all_refs, "S = 1, mask lifted")
        ix.set_option("two_level_sub", 8)                    # no repack in between: the next query builds the copy again
        ix.set_option("two_level_sub_rank", 1)
        _, _, ri = _check(ix, X2, oracle.knn(X2, Y2, K, 0, nthreads=16), 300, all_refs, "S = 8 ranked by index, no repack")
        ix.set_ref(Y1)
        ix.set_option("two_level_sub_rank", 0)
        _, _, r8b = _check(ix, X1, oracle.knn(X1, Y1, K, 0, nthreads=16), 700, all_refs, "set_ref(Y1) again, S = 8")
    finally:
        ix.close()
    assert np.array_equal(r8, r8b), "the same references, the same S: the same order"
    assert not np.array_equal(r1, ri)


def test_cosine_with_every_reference_in_one_bucket(gpu_lib):
    """the four anchor cells are the same cell: one bucket of 5000 references, the other three empty"""
    X, Y = _pca(5000, 300, 81)
    Yd = Y.copy()
    Yd[1250::1250][:3] = Yd[0]
    _sweep(gpu_lib, X, Yd, "one bucket, cosine", metric=2)


def test_the_self_drop(gpu_lib):
    _, Y = _pca(5000, 700, 11)
    _sweep(gpu_lib, Y[:700].copy(), Y, "rows among the references, themselves dropped", drop=True, k=K - 1)      # (k' = k + 1 = 15)


def test_two_loopback_shard_ranks(gpu_lib):
    """each rank's candidate query is planned on the two-level slot order with local seeds; the sub-order's option is set on
    both ranks and the sharded result equals the oracle's over all 10000 references"""
    from nabo_amd import _sharded
    X, Y = _pca(10000, 300, 41)
    grp = _sharded.ShardedGroup([0, 0], 10000, G, 0, Y, transport="loopback")
    try:
        for ix in grp.indices:
            for name, value in dict(TL, two_level_sub=8).items():
                ix.set_option(name, value)
        grp.set_ref()
        gi, gd = grp.query(X, K)
    finally:
        grp.close()
    oi, od = oracle.knn(X, Y, K, 0, nthreads=16)
    assert np.array_equal(gi, oi) and gd.tobytes() == od.tobytes()
