"""The two-level stream of the one-product pass (nabo_amd/csrc/l2c_topk.hip, slot order nabo_amd/csrc/l2c_slots.h): targets and
references are streamed in bucket order, a tile's first operand step alone bounds its scores from below, and only a tile
with a bound below some row's threshold gets its second step.  No pair is skipped and a bound never exceeds its score, so
every result must be the oracle's bits -- all rows are compared.

Option "two_level" = 2 takes the path below the sizes the planner would ("splits" = 1: it serves one-split launches;
"local_anchors" = 4: buckets of about a thousand references).  The base shape is 700 rows (no multiple of a wave's 96) over
5000 references (no multiple of a tile's 32), k = 15, d = 50.  The tile counters of nabo_index_last_kernel (last_stats keys
two_level_*) show that both loops ran: clustered data runs one-step tiles and refetches some, one broad cloud sends the
waves back to the two-step loop."""
import functools

import numpy as np
import pytest

import oracle
from nabo_amd import _knn
from nabo_amd._synth import pca_like

pytestmark = pytest.mark.gpu

TL = {"two_level": 2, "splits": 1, "local_anchors": 4}
M, N, K = 700, 5000, 15


@functools.lru_cache(maxsize=None)
def _pca(n, g, m, seed):
    Y, X = pca_like(n, g, seed=seed), pca_like(m, g, seed=seed + 1)
    Y.setflags(write=False)
    X.setflags(write=False)
    return X, Y


def _run(gpu_lib, X, Y, k=K, mask=None, opts=TL):
    """the query with the two-level stream against the oracle, every row; returns the statistics and the kernel's name"""
    oi, od = oracle.knn(X, Y, k, 0, ref_mask=mask, nthreads=8)
    ix = gpu_lib.KnnIndex(Y.shape[0], Y.shape[1], options=opts).set_ref(Y, ref_mask=mask)
    gi, gd = ix.query(X, k)
    st, kern = ix.last_stats(), ix.last_kernel()
    ix.close()
    assert np.array_equal(gi, oi) and np.array_equal(gd, od), int((gi != oi).any(axis=1).sum())
    assert kern.startswith("l2c_topk_kernel<2,1,23,6,32,4,2>") and "two-level tiles" in kern, kern
    print({a: b for a, b in st.items() if a.startswith("two_level") or a.endswith("_rows")})
    return st


def test_the_planner_reports_the_decision():
    assert _knn.query_plan(N, 50, M, K, options=TL)["two_level"] == 2
    assert _knn.query_plan(N, 50, M, K, options=dict(TL, two_level=0))["two_level"] == 0
    assert _knn.query_plan(N, 50, M, K, options={"splits": 1})["two_level"] == 0            # by default only where local seeds are
    assert _knn.query_plan(N, 50, M, K, options={"two_level": 2})["two_level"] == 1          # reference splits: the slot order only
    assert _knn.query_plan(1000000, 50, 1000000, K)["two_level"] == 2
    for g, want in ((28, 0), (29, 2), (59, 2), (60, 0)):
        p = _knn.query_plan(N, g, M, K, options=TL)
        assert p["two_level"] == want and p["kernel"].startswith("l2c_topk_kernel<2," if g > 28 else "l2c_topk_kernel<1,"), (g, p)


def test_clustered_data_runs_one_step_tiles_and_refetches_some(gpu_lib):
    X, Y = _pca(N, 50, M, 11)
    st = _run(gpu_lib, X, Y)
    assert st["two_level_one_step_tiles"] > 0 and st["two_level_refetched_tiles"] > 0, st


def test_one_gaussian_cloud_falls_back_to_the_two_step_loop(gpu_lib):
    rng = np.random.default_rng(5)
    Y, X = rng.standard_normal((N, 50)), rng.standard_normal((M, 50))
    st = _run(gpu_lib, X, Y)
    assert st["two_level_two_step_tiles"] > st["two_level_one_step_tiles"] > 0, st


def test_tight_clusters_far_from_the_centre_go_down_the_pass_chain(gpu_lib):
    """clusters of unit width 800 widths from the centre of the data: the one-product bound 2^-9 ||x|| ||y|| dwarfs the
    distances inside a cluster, the first pass certifies little and the passes behind it answer"""
    rng = np.random.default_rng(6)
    centres = rng.standard_normal((8, 50))
    centres *= 800.0 / np.linalg.norm(centres, axis=1, keepdims=True)
    Y = centres[rng.integers(0, 8, N)] + rng.standard_normal((N, 50))
    X = centres[rng.integers(0, 8, M)] + rng.standard_normal((M, 50))
    st = _run(gpu_lib, X, Y)
    assert st["seeded_pass_rows"] + st["second_pass_rows"] + st["fallback_rows"] > 0, st


def test_a_lattice_with_exact_ties_and_duplicated_references(gpu_lib):
    rng = np.random.default_rng(7)
    L = rng.integers(0, 3, (N - 500, 50)).astype(np.float64)
    Y = np.concatenate([L, L[:500]])
    X = np.concatenate([L[100:100 + M // 2], rng.integers(0, 3, (M - M // 2, 50)).astype(np.float64)])
    _run(gpu_lib, X, Y)


def test_a_masked_third_of_the_references_and_a_one_row_query(gpu_lib):
    X, Y = _pca(N, 50, M, 11)
    mask = np.zeros(N, dtype=np.uint8)
    mask[::3] = 1
    _run(gpu_lib, X, Y, mask=mask)
    _run(gpu_lib, X[5:6], Y)


M_MEMORY = 1100         # at least 1024 rows (the memory's bound), no multiple of a wave's 96 rows or a workgroup's 384


@functools.lru_cache(maxsize=None)
def _memory_case(name):
    """the two seeded data sets of the memory test with the oracle's answer for all M_MEMORY rows (a shorter query: a prefix)"""
    if name == "clustered":
        # four tight clusters of 1250 cells, one anchor cell (0, 1250, 2500, 3750) in each: the file's pca_like data leaves the
        # verdict "no" at this shape just as the cloud does (seed 11: one-step 344, two-step 1600)
        rng = np.random.default_rng(17)
        centres = 20.0 * np.eye(4, 50)
        Y = centres[np.repeat([0, 1, 2, 3], N // 4)] + rng.standard_normal((N, 50))
        X = centres[rng.integers(0, 4, M_MEMORY)] + rng.standard_normal((M_MEMORY, 50))
    else:
        rng = np.random.default_rng(5)
        Y, X = rng.standard_normal((N, 50)), rng.standard_normal((M_MEMORY, 50))
    oi, od = oracle.knn(X, Y, K, 0, nthreads=8)
    for a in (X, Y, oi, od):
        a.setflags(write=False)
    return X, Y, oi, od


def _memory_query(ix, X, oi, od):
    """one query against the oracle, every row; returns (the stream ran, what its counters make the memory say: it stays)"""
    gi, gd = ix.query(X, K)
    st, kern = ix.last_stats(), ix.last_kernel()
    assert np.array_equal(gi, oi[:len(X)]) and np.array_equal(gd, od[:len(X)]), int((gi != oi[:len(X)]).any(axis=1).sum())
    one, two = st["two_level_one_step_tiles"], st["two_level_two_step_tiles"]
    print(len(X), "streamed" if "two-level tiles" in kern else "caller order", "one-step", one, "two-step", two)
    return "two-level tiles" in kern, not one * 3 < two


def test_the_memory_a_launch_leaves(gpu_lib):
    """A launch of the stream whose waves ran fewer than a quarter of their tiles one-step (one_step * 3 < two_step) leaves
    the verdict "no" (nabo_amd/csrc/two_level_verdict.h): the next query runs caller order -- from 1024 rows on; the verdict
    outlives 15 further set_ref calls and is forgotten at the 16th.  Counters of the first query of M_MEMORY rows at the
    commit before the verdict got its header: four tight clusters one-step 1728, two-step 540 (stays; 1000 rows: 1314 and
    468); one cloud one-step 240, two-step 1704 (leaves; 1000 rows: the same, and both queries stream)."""
    outcomes = set()
    for name in ("clustered", "cloud"):
        X, Y, oi, od = _memory_case(name)
        ix = gpu_lib.KnnIndex(N, 50, options=TL).set_ref(Y)
        streamed, stays = _memory_query(ix, X, oi, od)
        assert streamed
        outcomes.add(stays)
        assert _memory_query(ix, X, oi, od)[0] == stays, name
        if not stays:
            for _ in range(15):
                ix.set_ref(Y)
            assert not _memory_query(ix, X, oi, od)[0]          # the verdict outlives 15 repacks ...
            ix.set_ref(Y)
            assert _memory_query(ix, X, oi, od)[0]              # ... and not the 16th
        ix.close()
        # below 1024 rows the rule is off: both queries stream, whatever the counters say
        ix = gpu_lib.KnnIndex(N, 50, options=TL).set_ref(Y)
        assert _memory_query(ix, X[:1000], oi, od)[0] and _memory_query(ix, X[:1000], oi, od)[0], name
        ix.close()
    assert outcomes == {True, False}, outcomes


@pytest.mark.parametrize("g", [29, 59, 28, 60])
def test_the_edges_in_d(gpu_lib, g):
    """one tail component, the last eligible d, and on either side a d the old path serves"""
    X, Y = _pca(N, g, M, 21)
    oi, od = oracle.knn(X, Y, K, 0, nthreads=8)
    ix = gpu_lib.KnnIndex(N, g, options=TL).set_ref(Y)
    gi, gd = ix.query(X, K)
    st = ix.last_stats()
    ix.close()
    assert np.array_equal(gi, oi) and np.array_equal(gd, od)
    ran = st["two_level_one_step_tiles"] + st["two_level_two_step_tiles"] > 0
    assert ran == (g in (29, 59)) == (_knn.query_plan(N, g, M, K, options=TL)["two_level"] == 2), st
