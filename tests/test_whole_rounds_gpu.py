"""The partition of a query whose two-level main launch comes with a tail launch (nabo_amd/csrc/plan.hip, query.hip): the main
launch takes as many rows as fit its workgroups as POSITIONS of the bucket-ordered copy, the tail launch begins there -- no
longer at a multiple of a workgroup's rows.  The smallest shape the planner gives such a pair: 200 000 rows (one round of
512 workgroups and a remainder) over a reference stream just long enough for a tail launch (256 tiles), no multiple of a
tile.  Compared with the oracle's bits: every row of the tail launch, every row within 1 000 of the cut, and a seeded sample
of 2 000 others; then once more on the same index after set_ref with other data (the buffers of the first query, reused
with the moved first row of the tail).

With four buckets over this data most tiles need their second step, and an index remembers such an outcome: its next
queries would take the caller-order stream and the parent's partition.  Option "coarse_adapt" = 0 switches that memory
off, so that the second query runs the ordered launch on the moved cut again; the other test below covers an index that
decides against the stream."""
import numpy as np
import pytest

import oracle
from nabo_amd import _knn
from nabo_amd._synth import pca_like

pytestmark = pytest.mark.gpu

OPTS = {"two_level": 2, "local_anchors": 4, "coarse_adapt": 0}
N, M, G, K = 8219, 200000, 50, 15


def _rows_to_compare(plan):
    cut = plan["rows_main"]
    near = np.arange(max(0, cut - 1000), min(M, cut + 1000))
    tail = np.arange(cut, M)
    others = np.random.default_rng(17).choice(cut, 2000, replace=False)
    return np.unique(np.concatenate([near, tail, others]))


def test_every_row_of_the_tail_and_around_the_cut_is_the_oracles(gpu_lib):
    plan = _knn.query_plan(N, G, M, K, options=OPTS)
    print(plan)
    if not (plan["two_level"] == 2 and plan["workgroups_tail"] > 0 and plan["rows_main"] < plan["workgroups_main"] * plan["rows_per_wg"]):
        pytest.skip("the planner gives this shape no ordered main launch with a tail launch: %r" % (plan,))
    assert plan["rows_main"] % plan["rows_per_wg"] != 0, "the cut lies inside a workgroup of rows: what this test is about"
    rows = _rows_to_compare(plan)
    X = pca_like(M, G, seed=41)
    ix = gpu_lib.KnnIndex(N, G, options=OPTS)
    try:
        for seed in (42, 43):                                  # the second round: other references into the same index
            Y = pca_like(N, G, seed=seed)
            ix.set_ref(Y)
            gi, gd = ix.query(X, K)
            st, kern = ix.last_stats(), ix.last_kernel()
            assert "two-level tiles" in kern and st["two_level_one_step_tiles"] > 0, (seed, kern[-120:])
            oi, od = oracle.knn(X[rows], Y, K, 0, nthreads=16)
            bad = (gi[rows] != oi).any(axis=1) | (gd[rows] != od).any(axis=1)
            assert not bad.any(), (seed, int(bad.sum()), rows[bad][:10], plan["rows_main"])
    finally:
        ix.close()


def test_a_cloud_without_clusters_whose_probe_says_no_after_the_plan_was_made(gpu_lib):
    """Default options, the smallest reference set that takes the stream by default (2^18), one broad Gaussian cloud: the first
    query is planned on whole rounds, its probe decides against the stream, and the main part -- which now ends inside a
    workgroup of rows -- runs in caller order with the tail launch taking over at the cut.  The second query knows the verdict
    before it plans and keeps whole workgroups.  Both: rows around both cuts, of both tails and a sample, against the oracle."""
    n, m = 262144 + 37, M
    plan = _knn.query_plan(n, G, m, K)
    if not (plan["two_level"] == 2 and plan["workgroups_tail"] > 0 and plan["rows_main"] < plan["workgroups_main"] * plan["rows_per_wg"]):
        pytest.skip("the planner gives this shape no ordered main launch with a tail launch: %r" % (plan,))
    rng = np.random.default_rng(3)
    Y, X = rng.standard_normal((n, G)), rng.standard_normal((m, G))
    cuts = (plan["rows_main"], plan["workgroups_main"] * plan["rows_per_wg"])
    rows = np.unique(np.concatenate([np.arange(c - 150, c + 150) for c in cuts] + [np.arange(m - 300, m), rng.choice(m, 300, replace=False)]))
    oi, od = oracle.knn(X[rows], Y, K, 0, nthreads=16)
    ix = gpu_lib.KnnIndex(n, G).set_ref(Y)
    try:
        for _ in range(2):
            gi, gd = ix.query(X, K)
            assert "two-level tiles" not in ix.last_kernel(), ix.last_kernel()
            bad = (gi[rows] != oi).any(axis=1) | (gd[rows] != od).any(axis=1)
            assert not bad.any(), (int(bad.sum()), rows[bad][:10], cuts)
    finally:
        ix.close()
