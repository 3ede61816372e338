"""The two-level stream and the local seeds in the randomised sweep (include/nabo_knn.h: "every setting returns the SAME BITS").

tests/test_option_sweep_gpu.py draws from OPTION_NAMES[] of plan.hip and never reaches the bucket-ordered stream of the
one-product pass (l2c_topk.hip) nor the local seeds' buckets (local_seeds.hip).  The cases here come from
_option_sweep.stream_cases: every index starts with two_level = 2 on one reference split, over shapes from 4 references up,
d = 29..59, k + drop = 1..15 (now and then beyond, which leaves the stream on a resident index), the self-drop, the sweep's
data flavours and masks, the nine options of LOCAL_SEED_OPTION_NAMES[] and TWO_LEVEL_OPTION_NAMES[] with their clamps, the
main table's options on top, and a short script of set_option / set_mask / set_ref on the resident index.  Every query
must equal the oracle's bits (all rows) and a default index's, and across a metric's cases the stream must have run where
the planner said so: a sweep that quietly stops reaching the stream fails.  tests/test_option_table.py checks the planned
reach without a GPU.  A failure names its case; one line replays it:
    python tests/test_stream_sweep_gpu.py <metric> <seed> <case>

Below the sweep: fixed cases a draw cannot guarantee (as many anchors as references, a padded last tile, every reference in
one bucket under cosine, one resident index through set_ref / set_mask / two_level off and on, two loopback shard ranks)."""
import functools
import os
import sys
from collections import Counter

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import _option_sweep as S  # noqa: E402
import oracle  # noqa: E402
import test_option_sweep_gpu as O  # noqa: E402

pytestmark = pytest.mark.gpu

CHUNK = 8                                                  # cases of one test item
CHUNKS = [(seed, c) for seed in S.SEEDS for c in range(-(-S.STREAM_CASES // CHUNK))]
RAN = "two-level tiles"                                    # nabo_index_last_kernel of a query that ran the stream
TILES = ("two_level_one_step_tiles", "two_level_refetched_tiles", "two_level_two_step_tiles")


def _new_tally():
    return dict(O._tally(), planned=0, ran=0, tiles=Counter(), stream_pass=Counter(), centre=Counter(), done=set())


def _centre_in_force(case, step):
    """cosine_centre as the operands of the query at `step` were packed: the option's value at the last set_ref before it"""
    value = now = case["options"].get("cosine_centre", 1)
    for st in case["steps"][:step]:
        if st[0] == "set_option" and st[1] == "cosine_centre":
            now = st[2]
        elif st[0] == "set_ref":
            value = now
    return value


def _hook(tally):
    def on_query(case, step, opts, plan, stats, kern, row_pass):
        where = S.describe(case, step) + " options now=%s" % opts
        if plan["two_level"] != 2:
            assert RAN not in kern, "planned without the two-level stream, launched with it: %s\n%s" % (where, kern)
            return
        tally["planned"] += 1
        if RAN not in kern:
            return
        assert kern.startswith("l2c_topk_kernel<2,1,23,6,32,4,2>"), (where, kern)
        tally["ran"] += 1
        for t in TILES:
            tally["tiles"][t] += stats[t]
        for code, cnt in zip(*np.unique(row_pass, return_counts=True)):
            tally["stream_pass"][O.PASS[int(code)]] += int(cnt)
        tally["centre"][_centre_in_force(case, step)] += 1
    return on_query


def _run_chunk(tally, mp, metric, seed, chunk):
    for case in S.stream_cases(metric, seed)[chunk * CHUNK:(chunk + 1) * CHUNK]:
        O.run_case(case, mp, tally, on_query=_hook(tally))
    tally["done"].add((seed, chunk))


@pytest.fixture(scope="module")
def stream_tally():
    return {0: _new_tally(), 2: _new_tally()}


@pytest.mark.parametrize("seed,chunk", CHUNKS)
@pytest.mark.parametrize("metric", [0, 2])
def test_stream_cases_return_the_oracles_bits(gpu_lib, monkeypatch, stream_tally, metric, seed, chunk):
    _run_chunk(stream_tally[metric], monkeypatch, metric, seed, chunk)


@pytest.mark.parametrize("metric", [0, 2])
def test_the_sweep_ran_the_stream_where_it_was_planned(gpu_lib, monkeypatch, stream_tally, metric):
    """After the chunks of one metric (run here if they were deselected): the stream ran in at least half of the queries
    planned with it -- an index may decide against it after a long query whose waves ran most tiles two-step, and remembers
    that under coarse_adapt (tests/test_whole_rounds_gpu.py), so equality is not demanded --, all three tile counters moved,
    the pass chain behind the stream answered rows, and cosine ran it on centred and on plain operands."""
    tally = stream_tally[metric]
    for seed, chunk in CHUNKS:
        if (seed, chunk) not in tally["done"]:
            _run_chunk(tally, monkeypatch, metric, seed, chunk)
    print("metric %d: the stream ran in %d of the %d queries planned with it (%.1f %%); tiles %s; rows by pass behind the stream %s; "
          "cosine_centre %s; all rows by pass %s kernels %s" % (
              metric, tally["ran"], tally["planned"], 100.0 * tally["ran"] / max(1, tally["planned"]), dict(tally["tiles"]),
              dict(tally["stream_pass"]), dict(tally["centre"]), dict(tally["pass"]), dict(tally["kernel"])))
    assert tally["planned"] > 0 and 2 * tally["ran"] >= tally["planned"], (tally["ran"], tally["planned"])
    for t in TILES:
        assert tally["tiles"][t] > 0, dict(tally["tiles"])
    answered = {p for p, c in tally["stream_pass"].items() if c > 0}
    assert {"ONE_PRODUCT", "SEEDED", "SECOND"} <= answered, dict(tally["stream_pass"])
    if metric == 2:
        assert tally["centre"][0] > 0 and tally["centre"][1] > 0, dict(tally["centre"])


# ---- fixed cases the draw cannot guarantee ----------------------------------------------------------------------------

TL = {"two_level": 2, "splits": 1, "local_anchors": 4, "coarse_adapt": 0}
G = 50


@functools.lru_cache(maxsize=None)
def _pca(n, m, seed):
    from nabo_amd._synth import pca_like
    Y, X = pca_like(n, G, seed=seed), pca_like(m, G, seed=seed + 1)
    Y.setflags(write=False)
    X.setflags(write=False)
    return X, Y


def _query(ix, X, Y, k, metric, what, mask=None, drop=False, stream=True):
    """one query of a resident index against the oracle, every row; whether the stream ran; its statistics"""
    got = ix.query(X, k, drop_first=drop)
    st, kern = ix.last_stats(), ix.last_kernel()
    O._same(got, oracle.knn(X, Y, k, metric, ref_mask=mask, drop_first=drop, nthreads=16), what)
    assert (RAN in kern) == stream, (what, kern)
    return st


def _planned(n, m, k, metric, opts, drop=False):
    from nabo_amd import _knn
    return _knn.query_plan(n, G, m, k, metric=metric, drop_first=drop, options=opts)


@pytest.mark.parametrize("metric", [0, 2])
@pytest.mark.parametrize("n", [4, 64])
def test_as_many_anchors_as_references(gpu_lib, metric, n):
    """one cell per bucket: k = 1 and k = n (n = 64: beyond the filter kernels, the exact route on the same index), and the
    self-drop with every other reference as a neighbour"""
    opts = dict(TL, local_anchors=n)
    X, Y = _pca(n, 97, 60 + n)
    for k in (1, n):
        p = _planned(n, 97, k, metric, opts)
        assert (p["two_level"], p["local_seed_buckets"]) == ((2, n) if k <= S.STREAM_MAX_KK else (0, 0)), p
    ix = gpu_lib.KnnIndex(n, G, metric=metric, options=opts).set_ref(Y)
    try:
        _query(ix, X, Y, 1, metric, "n = anchors = %d, k = 1" % n)
        _query(ix, X, Y, n, metric, "n = anchors = %d, k = n" % n, stream=n <= S.STREAM_MAX_KK)
        _query(ix, X, Y, 1, metric, "n = anchors = %d, k = 1 again" % n)
        kd = min(n - 1, S.STREAM_MAX_KK - 1)
        _query(ix, Y, Y, kd, metric, "n = anchors = %d, self-drop, k = %d" % (n, kd), drop=True)
    finally:
        ix.close()


@pytest.mark.parametrize("metric", [0, 2])
def test_a_padded_last_tile(gpu_lib, metric):
    """33 references: the second tile holds one cell and 31 slots of padding; 97 rows: a wave and one row"""
    X, Y = _pca(33, 97, 71)
    assert _planned(33, 97, 15, metric, TL)["two_level"] == 2
    ix = gpu_lib.KnnIndex(33, G, metric=metric, options=TL).set_ref(Y)
    try:
        _query(ix, X, Y, 15, metric, "n = 33, 4 anchors")
        mask = np.zeros(33, dtype=np.uint8)
        mask[[0, 31]] = 1
        ix.set_mask(mask)
        _query(ix, X, Y, 15, metric, "n = 33, 4 anchors, cells 0 and 31 masked", mask=mask)
    finally:
        ix.close()


def test_all_references_in_one_bucket_under_cosine(gpu_lib):
    """Duplicated anchor cells (tests/test_local_seeds_gpu.py): every anchor is the same point, ties go to the lowest anchor,
    bucket 0 holds every reference and the three others are empty -- and with local_cap = 2048 only its first 2048 cells."""
    X, Y = _pca(5000, 300, 11)
    Yd = Y.copy()
    Yd[1250::1250][:3] = Yd[0]                               # the anchors are the cells 0, 1250, 2500, 3750
    for opts in (TL, dict(TL, local_cap=2048)):
        assert _planned(5000, 300, 15, 2, opts)["two_level"] == 2
        ix = gpu_lib.KnnIndex(5000, G, metric=2, options=opts).set_ref(Yd)
        try:
            _query(ix, X, Yd, 15, 2, "one bucket, cosine, %s" % opts)
        finally:
            ix.close()


@pytest.mark.parametrize("metric", [0, 2])
def test_one_resident_index_through_new_references_masks_and_the_switch(gpu_lib, metric):
    """The anchors, the runs, the bucket ends and the ordered copies follow set_ref and set_mask; two_level = 0 leaves the
    stream and two_level = 2 returns to it.  coarse_adapt = 0: the index keeps no memory of a query's outcome."""
    X1, Y1 = _pca(5000, 700, 11)
    X2, Y2 = _pca(5000, 700, 81)
    X2, Y2 = X2 * 1e3 + 3.0, Y2 * 1e3 + 3.0
    mask = np.zeros(5000, dtype=np.uint8)
    mask[::3] = 1
    mask[1250] = mask[2500] = 1                              # two of the four anchor cells among them
    ix = gpu_lib.KnnIndex(5000, G, metric=metric, options=TL)
    try:
        ix.set_ref(Y1)
        _query(ix, X1, Y1, 15, metric, "set_ref(Y1)")
        ix.set_mask(mask)
        _query(ix, X1, Y1, 15, metric, "set_mask", mask=mask)
        ix.set_ref(Y2, ref_mask=mask)
        _query(ix, X2, Y2, 15, metric, "set_ref(Y2)", mask=mask)
        ix.set_mask(None)
        _query(ix, X2, Y2, 15, metric, "set_mask(None)")
        ix.set_option("two_level", 0)
        _query(ix, X2, Y2, 15, metric, "two_level = 0", stream=False)
        ix.set_option("two_level", 2)
        st = _query(ix, X2, Y2, 15, metric, "two_level = 2 again")
        assert st["two_level_one_step_tiles"] + st["two_level_two_step_tiles"] > 0, st
    finally:
        ix.close()


@pytest.mark.parametrize("metric", [0, 2])
def test_two_loopback_shard_ranks(gpu_lib, metric):
    """Each rank's candidate query over its 5000 references is planned on the two-level slot order with local seeds (the
    stream itself serves full queries only): the sharded result equals the oracle's over all 10000."""
    from nabo_amd import _knn, _sharded
    X, Y = _pca(10000, 300, 41)
    opts = {"two_level": 2, "splits": 1, "local_anchors": 4}
    n_cand = _sharded.candidates_per_shard(15, 2, 300)
    p = _knn.query_plan(5000, G, 300, 15, metric=metric, n_cand=n_cand, options=opts)
    assert p["two_level"] == 1 and p["local_seed_buckets"] == 4, p
    grp = _sharded.ShardedGroup([0, 0], 10000, G, metric, Y, transport="loopback")
    try:
        for ix in grp.indices:
            for name, value in opts.items():
                ix.set_option(name, value)
        grp.set_ref()
        got = grp.query(X, 15)
    finally:
        grp.close()
    O._same(got, oracle.knn(X, Y, 15, metric, nthreads=16), "two loopback shard ranks, metric %d" % metric)


if __name__ == "__main__":                       # replay one case: python tests/test_stream_sweep_gpu.py metric seed case
    metric, seed, number = (int(a) for a in sys.argv[1:4])
    case = S.stream_cases(metric, seed)[number]
    print(S.describe(case))
    with pytest.MonkeyPatch.context() as mp:
        t = _new_tally()
        O.run_case(case, mp, t, on_query=_hook(t))
    print("equal to the oracle; the stream ran in %d of the %d queries planned with it; tiles %s; rows by pass %s kernels %s" % (
        t["ran"], t["planned"], dict(t["tiles"]), dict(t["pass"]), dict(t["kernel"])))
