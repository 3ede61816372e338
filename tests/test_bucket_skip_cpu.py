"""Which sub-buckets of the two-level stream a workgroup skips, without a GPU: the rule of nabo_amd/csrc/bucket_skip.h
(compiled here with g++ through tests/bucket_skip_host, assembled there as the kernels assemble it) against a numpy
restatement, and against float64 brute force.

The rule: references are cut into buckets (nearest of C strided anchor cells) and sub-buckets (nearest of S strided
sub-anchors of the bucket; a bucket with fewer than S cells is one group).  With u[b][b'] the unit vector from the mean of
bucket b to the mean of b', a group of b' lies out of reach of a row of bucket b with start threshold tau0 when
min over the group of y.u[b][b'] - x.u[b][b'] >= sqrt(tau0 + ||x||^2); a workgroup of 384 positions skips a group when that
holds for every live row, and never a group of its rows' own buckets.  What must hold whatever the rounding: NO skipped
(row, reference) pair has ||x - y||^2 - ||x||^2 < tau0."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from nabo_amd import _knn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LKEEP, WG = 23, 384
vp = C.c_void_p


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("bskip") / "libbskip_host.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-fPIC", "-shared",
                           "-I" + os.path.join(REPO, "nabo_amd", "csrc"),
                           os.path.join(REPO, "tests", "bucket_skip_host", "skip_shim.cpp"), "-o", so])
    L = C.CDLL(so)
    L.bskip_float_below_host.restype = L.bskip_float_above_host.restype = C.c_float
    L.bskip_float_below_host.argtypes = L.bskip_float_above_host.argtypes = [C.c_double]
    L.bskip_refs_host.argtypes = [C.c_int64, C.c_int, vp, vp, C.c_double, vp, vp, C.c_int, C.c_int, vp, vp, vp]
    L.bskip_workgroup_host.argtypes = [C.c_int64, C.c_int, vp, vp, C.c_double, vp, vp, C.c_int, C.c_int, vp, vp, vp]
    L.bskip_group_tiles_host.argtypes = [C.c_int64, C.c_int64, vp, vp]
    L.bskip_build_runs_host.argtypes = [C.c_int, vp, vp, vp, C.c_int32, C.c_int, vp]
    L.bskip_kept_tiles_host.restype = C.c_int64
    L.bskip_kept_tiles_host.argtypes = [vp]
    L.bskip_buildable_host.argtypes = [C.c_int64, C.c_int]
    L.bskip_max_tiles_host.restype = C.c_int64
    return L


def _p(a):
    return a.ctypes.data_as(vp)


# ---- the data and the partition (a restatement of the bucket and sub-bucket rule, float64) ----
def _nearest(V, A):
    return np.argmin((A * A).sum(1)[None, :] - 2.0 * V @ A.T, axis=1)


def _partition(Y, nb, S, mask=None):
    """bucket [n] (-1 masked) and group [n] = bucket * S + sub-bucket"""
    n = len(Y)
    live = np.ones(n, bool) if mask is None else ~mask
    bucket = np.where(live, _nearest(Y, Y[np.arange(nb) * (n // nb)]), -1).astype(np.int32)
    group = np.full(n, -1, dtype=np.int32)
    for b in range(nb):
        idx = np.flatnonzero(bucket == b)
        sub = _nearest(Y[idx], Y[idx[np.arange(S) * (len(idx) // S)]]) if len(idx) >= S else np.zeros(len(idx), int)
        group[idx] = b * S + sub
    return bucket, group


def _clustered(n, m, d, seed, centres, spread=3.0):
    """`centres` clusters of unit width; the references lie cluster by cluster, so that each strided anchor cell falls into
    a cluster of its own when there are as many anchors as clusters"""
    rng = np.random.default_rng(seed)
    cen = spread * rng.standard_normal((centres, d))
    return cen[np.repeat(np.arange(centres), n // centres)] + rng.standard_normal((n, d)), cen[rng.integers(0, centres, m)] + rng.standard_normal((m, d))


def _case(name):
    d, S, mask = 50, 8, None
    if name == "cloud":
        rng = np.random.default_rng(3)
        Y, X, nb = rng.standard_normal((4000, d)), rng.standard_normal((600, d)), 4
    else:
        nb = 16 if name == "sixteen" else 4
        Y, X = _clustered(4000, 600, d, 1, nb)
    centre = Y.mean(0)
    scale = 2.0 ** 7
    if name == "small_and_empty":
        # bucket 1's anchor cell and all cells nearest to it but three are masked: fewer than S cells, one group; the cells
        # nearest to bucket 3's anchor are all masked: an empty bucket
        nb = 4
        b0, _ = _partition(Y, nb, S)
        mask = np.zeros(len(Y), bool)
        mask[np.flatnonzero(b0 == 1)[3:]] = True
        mask[b0 == 3] = True
    bucket, group = _partition(Y, nb, S, mask)
    if name == "small_and_empty":
        assert (bucket == 1).sum() == 3 and (bucket == 3).sum() == 0
    xb = _nearest(X, Y[np.arange(nb) * (len(Y) // nb)]).astype(np.int32)
    order = np.argsort(xb, kind="stable")
    X, xb = X[order], xb[order]
    Yt, Xt = (Y - centre) * scale, (X - centre) * scale
    # start thresholds: the 23rd smallest score among the references of the row's own bucket, as a float at or above it
    tau0 = np.full(len(X), np.inf, dtype=np.float32)
    for i in range(len(X)):
        own = Yt[bucket == xb[i]]
        if len(own) < LKEEP and name == "small_and_empty" and i % 2:
            own = Yt[bucket >= 0]                           # (any references bound the 23rd smallest score: every other such row has a seed)
        if len(own) >= LKEEP:
            s = np.sort(((own - Xt[i]) ** 2).sum(1) - (Xt[i] ** 2).sum())[LKEEP - 1]
            t = np.float32(s)
            tau0[i] = t if float(t) >= s else np.nextafter(t, np.float32(np.inf))
    return dict(X=X, Y=Y, Xt=Xt, Yt=Yt, centre=centre, scale=scale, nb=nb, S=S, bucket=bucket, group=group, xb=xb, tau0=tau0)


def _tables(L, c):
    nb, S, d = c["nb"], c["S"], c["Y"].shape[1]
    mean, u, ymin = np.zeros((nb, d)), np.zeros((nb, nb, d)), np.zeros((nb, nb * S), dtype=np.float32)
    L.bskip_refs_host(len(c["Y"]), d, _p(np.ascontiguousarray(c["Y"])), _p(c["centre"]), c["scale"], _p(c["bucket"]), _p(c["group"]), nb, S,
                      _p(mean), _p(u), _p(ymin))
    return mean, u, ymin


def _keep(L, c, u, ymin, rows, tau0=None):
    nb, S, d = c["nb"], c["S"], c["Y"].shape[1]
    keep = np.zeros(nb * S, dtype=np.uint8)
    X = np.ascontiguousarray(c["X"][rows])
    xb = np.ascontiguousarray(c["xb"][rows])
    t = np.ascontiguousarray((c["tau0"] if tau0 is None else tau0)[rows])
    own = L.bskip_workgroup_host(len(X), d, _p(X), _p(c["centre"]), c["scale"], _p(xb), _p(t), nb, S, _p(u), _p(ymin), _p(keep))
    return keep, own


def _restated(c, rows, tau0=None):
    """(keep [G], margin [G]): the rule in numpy, float64, no allowance; margin = the smallest slack over the rows"""
    nb, S = c["nb"], c["S"]
    Yt, Xt, bucket, group, xb = c["Yt"], c["Xt"][rows], c["bucket"], c["group"], c["xb"][rows]
    t = (c["tau0"] if tau0 is None else tau0)[rows].astype(np.float64)
    mean = np.array([Yt[bucket == b].mean(0) if (bucket == b).any() else np.zeros(Yt.shape[1]) for b in range(nb)])
    keep, margin = np.ones(nb * S, bool), np.full(nb * S, -np.inf)
    radius = np.sqrt(np.maximum(t + (Xt ** 2).sum(1), 0.0))
    for gi in range(nb * S):
        bp, members = gi // S, Yt[group == gi]
        if bp in xb or not np.isfinite(radius).all():
            continue
        slack = np.inf
        for b in np.unique(xb):
            diff = mean[bp] - mean[b]
            nrm = np.linalg.norm(diff)
            uu = diff / nrm if nrm > 0 and (bucket == b).any() and (bucket == bp).any() else np.zeros_like(diff)
            ymin = (members @ uu).min() if len(members) else np.inf
            r = Xt[xb == b]
            slack = min(slack, (ymin - r @ uu - radius[xb == b]).min())
        margin[gi] = slack
        keep[gi] = not slack >= 0.0
    return keep, margin


def _workgroups(c):
    m = len(c["X"])
    return [np.arange(s, min(s + WG, m)) for s in range(0, m, WG)]


@pytest.mark.parametrize("name", ["four", "sixteen", "small_and_empty", "cloud"])
def test_the_rule_agrees_with_its_restatement_and_skips_no_reachable_pair(shim, name):
    c = _case(name)
    mean, u, ymin = _tables(shim, c)
    nb, S = c["nb"], c["S"]
    for b in range(nb):
        members = c["Yt"][c["bucket"] == b]
        assert np.allclose(mean[b], members.mean(0) if len(members) else 0.0, rtol=1e-12, atol=1e-9)
        for bp in range(nb):
            nrm = np.linalg.norm(u[b, bp])
            assert nrm == 0.0 if (b == bp or not len(members) or not (c["bucket"] == bp).any()) else abs(nrm - 1.0) < 1e-12
    skipped_groups = 0
    for rows in _workgroups(c):
        keep, own = _keep(shim, c, u, ymin, rows)
        want, margin = _restated(c, rows)
        assert own == len(np.unique(c["xb"][rows]))
        clear = np.abs(margin) > 1e-6 * c["scale"]          # (the two sides sum in different orders and the header rounds outwards)
        assert np.array_equal(keep[clear] != 0, want[clear]), (name, np.flatnonzero((keep != 0) != want))
        assert all(keep[b * S:(b + 1) * S].all() for b in np.unique(c["xb"][rows]))          # the own buckets' groups stay
        Xt, t = c["Xt"][rows], c["tau0"][rows].astype(np.float64)
        for gi in np.flatnonzero(keep == 0):
            members = c["Yt"][c["group"] == gi]
            skipped_groups += len(members) > 0
            if len(members):
                score = ((Xt[:, None, :] - members[None, :, :]) ** 2).sum(2) - (Xt ** 2).sum(1)[:, None]
                assert (score >= t[:, None]).all(), (name, gi)
    if name in ("four", "sixteen"):
        assert skipped_groups > 0, name                     # clustered data: the rule does skip


def test_a_row_without_a_seed_vetoes_every_skip(shim):
    c = _case("four")
    _, u, ymin = _tables(shim, c)
    rows = _workgroups(c)[0]
    assert not _keep(shim, c, u, ymin, rows)[0].all()
    for bad in (np.inf, np.nan):
        tau0 = c["tau0"].copy()
        tau0[rows[17]] = bad
        assert _keep(shim, c, u, ymin, rows, tau0)[0].all(), bad


def test_padding_positions_do_not_count_and_too_many_own_buckets_veto(shim):
    c = _case("four")
    _, u, ymin = _tables(shim, c)
    rows = _workgroups(c)[0]
    keep, own = _keep(shim, c, u, ymin, rows)
    xb = c["xb"].copy()
    c2 = dict(c, xb=xb)
    xb[rows[::2]] = -1                                      # every other position is padding: fewer rows, no more kept
    keep2, _ = _keep(shim, c2, u, ymin, rows)
    assert (keep2 <= keep).all()
    xb[rows] = -1                                           # nothing but padding: nothing to run
    assert not _keep(shim, c2, u, ymin, rows)[0].any()
    consts = np.zeros(5, dtype=np.int64)
    shim.bskip_constants_host(_p(consts))
    assert list(consts) == [256, 514, 32, 384, 64]
    c16 = _case("sixteen")
    _, u16, ymin16 = _tables(shim, c16)
    assert _keep(shim, c16, u16, ymin16, np.arange(len(c16["X"])))[1] == len(np.unique(c16["xb"])) <= 32


def test_the_directed_roundings(shim):
    rng = np.random.default_rng(2)
    for v in list(rng.standard_normal(200) * 10.0 ** rng.integers(-30, 30, 200)) + [0.0, 1.0, -1.0, 1e-50, -1e-50, 1e39, -1e39]:
        lo, hi = shim.bskip_float_below_host(v), shim.bskip_float_above_host(v)
        assert float(lo) <= v <= float(hi), v
        assert float(np.nextafter(np.float32(lo), np.float32(np.inf))) > v or lo == hi
        assert float(np.nextafter(np.float32(hi), np.float32(-np.inf))) < v or lo == hi


# ---- the run list ----
def _runs(L, t0, t1, keep, t_end, cap):
    t0, t1, keep = np.asarray(t0, dtype=np.int32), np.asarray(t1, dtype=np.int32), np.asarray(keep, dtype=np.uint8)
    runs = np.full(2 * (cap + 1), -5, dtype=np.int32)
    n = L.bskip_build_runs_host(len(t0), _p(t0), _p(t1), _p(keep), t_end, cap, _p(runs))
    assert tuple(runs[2 * n:2 * n + 2]) == (0, 0)
    out = [(int(runs[2 * i]), int(runs[2 * i + 1])) for i in range(n)]
    assert L.bskip_kept_tiles_host(_p(runs)) == sum(e - b for b, e in out)
    return out


def _runs_restated(t0, t1, keep, t_end, cap):
    out = []
    for a, b, k in zip(t0, t1, keep):
        if not k or b <= a:
            continue
        a, b = a & ~1, min((b + 1) & ~1, t_end)
        if a >= b:
            continue
        if out and (a <= out[-1][1] or len(out) == cap):
            out[-1] = (out[-1][0], max(out[-1][1], b))
        else:
            out.append((a, b))
    return out


def _tiles(L, first, count):
    a, b = C.c_int32(), C.c_int32()
    L.bskip_group_tiles_host(first, count, C.byref(a), C.byref(b))
    return a.value, b.value


def test_group_tiles_and_the_edges_of_the_run_list(shim):
    assert _tiles(shim, 0, 0) == (0, 0) and _tiles(shim, 70, 0) == (2, 2)
    assert _tiles(shim, 0, 32) == (0, 1) and _tiles(shim, 31, 2) == (0, 2) and _tiles(shim, 64, 65) == (2, 5)
    # a sub-bucket ending on an odd tile: widened to the pair
    assert _runs(shim, [4], [7], [1], 40, 8) == [(4, 8)]
    assert _runs(shim, [5], [6], [1], 40, 8) == [(4, 6)]
    # two sub-buckets sharing a tile: the kept one keeps the shared tile; both kept: one run
    a, b = _tiles(shim, 100, 100), _tiles(shim, 200, 100)
    assert a == (3, 7) and b == (6, 10)
    assert _runs(shim, [a[0], b[0]], [a[1], b[1]], [0, 1], 40, 8) == [(6, 10)]
    assert _runs(shim, [a[0], b[0]], [a[1], b[1]], [1, 0], 40, 8) == [(2, 8)]
    assert _runs(shim, [a[0], b[0]], [a[1], b[1]], [1, 1], 40, 8) == [(2, 10)]
    # adjacent runs merge, a gap of one pair does not
    assert _runs(shim, [0, 4], [4, 6], [1, 1], 40, 8) == [(0, 6)]
    assert _runs(shim, [0, 6], [4, 8], [1, 1], 40, 8) == [(0, 4), (6, 8)]
    # a run at the very end of the stream, clipped to it; nothing kept: the sentinel alone
    assert _runs(shim, [36], [41], [1], 40, 8) == [(36, 40)]
    assert _runs(shim, [38], [39], [1], 40, 8) == [(38, 40)]
    assert _runs(shim, [0, 10], [3, 12], [0, 0], 40, 8) == []
    # empty groups keep nothing
    assert _runs(shim, [3, 3], [3, 5], [1, 1], 40, 8) == [(2, 6)]


def test_a_list_at_its_capacity_and_one_over_it(shim):
    cap = 5
    t0 = [4 * i for i in range(cap + 3)]
    t1 = [4 * i + 2 for i in range(cap + 3)]
    t_end = 4 * (cap + 3)
    full = [(4 * i, 4 * i + 2) for i in range(cap + 3)]
    assert _runs(shim, t0[:cap], t1[:cap], [1] * cap, t_end, cap) == full[:cap]                      # exactly at capacity: all kept apart
    over = _runs(shim, t0[:cap + 1], t1[:cap + 1], [1] * (cap + 1), t_end, cap)
    assert over == full[:cap - 1] + [(full[cap - 1][0], full[cap][1])]                              # one over: merged, not dropped
    more = _runs(shim, t0, t1, [1] * (cap + 3), t_end, cap)
    assert more == full[:cap - 1] + [(full[cap - 1][0], full[cap + 2][1])]
    rng = np.random.default_rng(9)
    for _ in range(200):
        ng = int(rng.integers(1, 40))
        first = np.sort(rng.integers(0, 3000, ng))
        count = np.minimum(rng.integers(0, 200, ng), np.append(np.diff(first), 200))
        tt = [_tiles(shim, int(f), int(n)) for f, n in zip(first, count)]
        keep = rng.integers(0, 2, ng)
        t_end = int(rng.integers(1, 55)) * 2
        cap = int(rng.integers(1, 12))
        got = _runs(shim, [a for a, _ in tt], [b for _, b in tt], keep, t_end, cap)
        assert got == _runs_restated([a for a, _ in tt], [b for _, b in tt], keep, t_end, cap)


# ---- where the skip is on: the option, the planner, and the ONE eligibility decision the reference build shares with it ----
def test_the_planner_reports_the_decision():
    M, N, K = 700, 5000, 15
    tl = {"two_level": 2, "splits": 1}
    assert _knn.query_plan(N, 50, M, K, options=dict(tl, bucket_skip=2))["bucket_skip"] == 1
    assert _knn.query_plan(N, 50, M, K, options=tl)["bucket_skip"] == 0               # a forced stream alone: no skip
    assert _knn.query_plan(N, 50, M, K, options=dict(tl, bucket_skip=1))["bucket_skip"] == 0
    assert _knn.query_plan(N, 50, M, K, options={"bucket_skip": 2})["bucket_skip"] == 0   # no stream, nothing to skip
    assert _knn.query_plan(1000000, 50, 1000000, K)["bucket_skip"] == 1              # the stream at its default setting
    assert _knn.query_plan(1000000, 50, 1000000, K, options={"bucket_skip": 1})["bucket_skip"] == 0
    assert _knn.query_plan(1000000, 50, 1000000, K, options={"two_level": 0})["bucket_skip"] == 0
    assert _knn.query_plan(1000000, 50, 1000000, K, options={"bucket_skip": 7})["bucket_skip"] == 1   # clamped to 2


def test_the_option_and_the_buildable_limits(shim):
    for option in (0, 1, 2):
        for tl_main in (0, 1):
            for two_level in (0, 1, 2):
                want = bool(tl_main) and option != 1 and (option == 2 or two_level == 1)
                assert bool(shim.bskip_planned_host(option, tl_main, two_level)) == want, (option, tl_main, two_level)
    top = shim.bskip_max_tiles_host()
    assert top == 1 << 19
    assert shim.bskip_buildable_host(2, 29) and shim.bskip_buildable_host(top, 64)
    assert not shim.bskip_buildable_host(top + 2, 50) and not shim.bskip_buildable_host(1000, 65) and not shim.bskip_buildable_host(0, 50)


def test_an_index_too_long_for_the_tables_never_plans_the_skip():
    """The reference build asks the same question as the planner (plan.hip: bskip_wanted): an index whose ordered copy has
    more than 2^19 tiles gets no tables, is never declared stale for want of them, and its plan shows no skip -- while it
    still takes the stream.  The last length with tables and the first without: the copy has ceil(n / 32) + 64 + 1 tiles, rounded down to even."""
    K, g, m = 15, 50, 1000000
    fits, too_long = ((1 << 19) - 64) * 32, ((1 << 19) - 63) * 32
    for n, want in ((fits, 1), (too_long, 0), (20000000, 0)):
        p = _knn.query_plan(n, g, m, K)
        assert p["two_level"] == 2 and p["bucket_skip"] == want, (n, p)
        assert _knn.query_plan(n, g, m, K, options={"bucket_skip": 2})["bucket_skip"] == want
