"""Every index option and filter mode against the oracle (include/nabo_knn.h: "every setting returns the SAME BITS").

The cases come from tests/_option_sweep.py: options, NABO_L2_MODE / NABO_CANBERRA_MODE, shapes, data flavours and a short
script of calls on one resident index (queries, set_option, set_mask, set_ref with other data).  Every query must equal
the oracle's bits and a default index's on the same data, and across a metric's cases every pass and filter kernel must
have answered rows: a sweep that quietly stops reaching a pass fails.  A failure names its case; one line replays it:
    python tests/test_option_sweep_gpu.py <metric> <seed> <case>

These cases never reach the two-level stream or the local seeds; tests/test_stream_sweep_gpu.py plays _option_sweep's
stream_cases through run_case below for those."""
import os
import sys
from collections import Counter

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import _option_sweep as S  # noqa: E402
import oracle  # noqa: E402

pytestmark = pytest.mark.gpu

PASS = {0: "ONE_PRODUCT", 1: "SEEDED", 2: "SECOND", 3: "WIDE", 4: "EXACT", 5: "CANBERRA"}   # NABO_PASS_*


def _same(got, want, what):
    gi, gd = got
    oi, od = want
    if np.array_equal(gi, oi) and np.array_equal(gd, od, equal_nan=True):
        return
    bad = np.nonzero((gi != oi).any(1) | ~((gd == od) | (np.isnan(gd) & np.isnan(od))).all(1))[0]
    r = int(bad[0])
    raise AssertionError("%s: %d of %d rows differ; row %d\n got  %s %s\n want %s %s" % (what, len(bad), len(gi), r, gi[r], gd[r],
                                                                                        oi[r], od[r]))


def _index(case, mp, options, with_mode=True):
    """A KnnIndex of the case's shape; the mode variable is set around nabo_index_create only (it is read there, once)."""
    import nabo_amd
    env = S.mode_env(case) if with_mode else None
    for var in ("NABO_L2_MODE", "NABO_CANBERRA_MODE"):
        mp.delenv(var, raising=False)
    if env:
        mp.setenv(*env)
    try:
        return nabo_amd.KnnIndex(case["n"], case["g"], metric=case["metric"], dist_factor=case["dist_factor"], options=options)
    finally:
        if env:
            mp.delenv(env[0])


def run_case(case, mp, tally, on_query=None):
    """Play the case's script on an index with its options and mode and on a default index; compare every query.
    on_query(case, step, options now, plan, last_stats(), last_kernel(), last_row_pass()) sees every query that passed."""
    from nabo_amd import _knn
    metric, n, g, f = case["metric"], case["n"], case["g"], case["dist_factor"]
    opts = dict(case["options"])
    ix, dflt = _index(case, mp, opts), _index(case, mp, {}, with_mode=False)
    try:
        variant = None
        Y = S.make_ref(case, variant)
        mask = S.make_mask(case["mask"], n, case["mask_seed"])
        for h in (ix, dflt):
            h.set_ref(Y, ref_mask=mask)
        for i, st in enumerate(case["steps"]):
            where = S.describe(case, i) + " options now=%s" % opts
            if st[0] == "set_option":
                ix.set_option(st[1], st[2])
                opts[st[1]] = st[2]
            elif st[0] == "set_mask":
                mask = S.make_mask(st[1], n, st[2])
                for h in (ix, dflt):
                    h.set_mask(mask)
            elif st[0] == "set_ref":
                variant = st[1]
                Y = S.make_ref(case, variant)
                for h in (ix, dflt):
                    h.set_ref(Y, ref_mask=mask)
            else:
                _, m, k, drop = st
                X = S.make_targets(case, variant, Y, m, drop, 1000 * case["case"] + i)
                got = ix.query(X, k, drop_first=drop)
                rp, kern = ix.last_row_pass(m), ix.last_kernel()
                stats = ix.last_stats() if on_query else None
                want = oracle.knn(X, Y, k, metric, f, ref_mask=mask, drop_first=drop, nthreads=16)
                _same(got, want, "oracle: " + where)
                _same(got, dflt.query(X, k, drop_first=drop), "default index: " + where)
                for code, cnt in zip(*np.unique(rp, return_counts=True)):
                    tally["pass"][PASS[int(code)]] += int(cnt)
                tally["kernel"][kern.split("<")[0].split(" ")[0]] += 1
                if metric != 1 and kern.startswith("l2c_topk_kernel"):
                    plan = _knn.query_plan(n, g, m, k, metric=metric, drop_first=drop, l2_mode=case["mode"], options=opts)
                    tally["geometry"][plan["geometry"]] += 1
                if on_query:
                    plan = _knn.query_plan(n, g, m, k, metric=metric, drop_first=drop, l2_mode=case["mode"], options=opts)
                    on_query(case, i, dict(opts), plan, stats, kern, rp)
    finally:
        ix.close()
        dflt.close()


def _tally():
    return {"pass": Counter(), "kernel": Counter(), "geometry": Counter()}


@pytest.mark.parametrize("metric", [0, 2, 1])
def test_every_option_and_mode_returns_the_oracles_bits(gpu_lib, monkeypatch, metric):
    tally = _tally()
    for seed in S.SEEDS:
        for case in S.cases(metric, seed):
            run_case(case, monkeypatch, tally)
    print("metric %d rows by pass %s kernels %s geometries %s" % (metric, dict(tally["pass"]), dict(tally["kernel"]),
                                                                  dict(tally["geometry"])))
    if metric == 1:
        need_pass, need_kern = {"CANBERRA", "EXACT"}, {"canberra_topk_kernel", "cbf_filter_kernel", "cbb_filter_kernel"}
    else:
        need_pass = {"ONE_PRODUCT", "SEEDED", "SECOND", "WIDE", "EXACT"}
        need_kern = {"l2c_topk_kernel", "l2q_topk_kernel", "l2_topk_kernel"}
        assert {0, 1, 2} <= set(tally["geometry"]), "one-product geometries that ran: %s" % dict(tally["geometry"])
    assert need_pass <= {p for p, c in tally["pass"].items() if c > 0}, "passes that answered rows: %s" % dict(tally["pass"])
    assert need_kern <= set(tally["kernel"]), "kernels that ran: %s" % dict(tally["kernel"])


@pytest.mark.parametrize("name", [c["name"] for c in S.large_cases()])
def test_large_cases_on_sampled_rows(gpu_lib, monkeypatch, name):
    """The long-stream one-round plan with its tail launch, the cost model's tail launch, a seeded pass on four splits:
    all rows equal a default index's, sampled rows -- every row of a rare pass among them -- equal the oracle's."""
    case = dict({"mode": None, "dist_factor": 0.25, "case": 0}, **next(c for c in S.large_cases() if c["name"] == name))
    n, g, m, k, drop, metric = case["n"], case["g"], case["m"], case["k"], case["drop"], case["metric"]
    Y = S.make_ref(case)
    X = S.make_targets(case, None, Y, m, drop, 1)
    mask = S.make_mask(case.get("mask"), n, 5)
    ix, dflt = _index(case, monkeypatch, case["options"]), _index(case, monkeypatch, {})
    try:
        ix.set_ref(Y, ref_mask=mask)
        dflt.set_ref(Y, ref_mask=mask)
        got = ix.query(X, k, drop_first=drop)
        rp, st = ix.last_row_pass(m), ix.last_stats()
        _same(got, dflt.query(X, k, drop_first=drop), "default index: %s" % name)
    finally:
        ix.close()
        dflt.close()
    from nabo_amd import _knn
    plan = _knn.query_plan(n, g, m, k, metric=metric, drop_first=drop, l2_mode=case["mode"], options=case["options"])
    if "tail" in name:
        assert plan["workgroups_tail"] > 0, plan
    if name == "seeded_pass_four_splits":
        assert st["seeded_pass_rows"] > 0 and st["list_len"] == 64, (np.bincount(rp, minlength=6), st)
    rng = np.random.default_rng(7)
    rare = np.nonzero(rp != np.bincount(rp).argmax())[0]
    rows = np.union1d(rng.choice(m, 300, replace=False), rng.permutation(rare)[:200])
    if plan["workgroups_tail"] > 0:                      # the tail launch's rows: the last workgroups' columns
        rows = np.union1d(rows, np.arange(max(0, m - 100), m))
    want = oracle.knn(X[rows], Y, k, metric, 0.25, ref_mask=mask, drop_first=drop, nthreads=16)
    _same((got[0][rows], got[1][rows]), want, "oracle: %s (sampled rows)" % name)


@pytest.mark.parametrize("metric", [0, 2])
def test_candidate_mode_under_cand_slack_and_masks(gpu_lib, metric):
    """nabo_index_query_candidates with cand_slack -1 / 0 / 3 / 8 (and reference splits, a geometry pin), masked references.
    What the global certification of nabo_sharded_query relies on holds for every setting: emitted entries carry their
    exact float64 distances in canonical order, the bound is a true lower bound on every reference not emitted, and the
    entries below the bound are exactly the head of the order row.  With the sharded query's own slack (-1) the whole
    emitted list is that head (test_knn_gpu.py: test_shard_candidates_and_their_bound); with cand_slack = 0 the list is
    the n_cand best one-product scores and its bound the one-product threshold, so only its certified part is."""
    from nabo_amd import _knn
    from nabo_amd._synth import pca_like
    for n, g, m, extra in ((6001, 30, 513, {}), (9000, 61, 300, {"splits": 5}), (4000, 100, 200, {"l2c_geo": 2})):
        Y = pca_like(n, g, seed=n + g)
        X = pca_like(m, g, seed=n + g + 1)
        mask = np.zeros(n, dtype=np.uint8)
        mask[::7] = 1
        full_i, full_d = oracle.knn(X, Y, 40, metric, ref_mask=mask, nthreads=16)
        D = oracle.pairwise(X, Y, metric, nthreads=16)
        dx = _knn.DeviceBuffer(X.nbytes).upload(X)
        for slack in (-1, 0, 3, 8):
            ix = gpu_lib.KnnIndex(n, g, metric=metric, ref_index_base=1000, options=dict(extra, cand_slack=slack))
            ix.set_ref(Y, ref_mask=mask)
            for nc in (1, 9, 16, 32):
                what = "n=%d g=%d m=%d options=%s n_cand=%d" % (n, g, m, dict(extra, cand_slack=slack), nc)
                di, dd, db = _knn.DeviceBuffer(m * nc * 8), _knn.DeviceBuffer(m * nc * 8), _knn.DeviceBuffer(m * 8)
                ix.query_candidates_device(dx.ptr, m, nc, di.ptr, dd.ptr, db.ptr)
                ci, cd, cb = di.download((m, nc), np.int64), dd.download((m, nc), np.float64), db.download((m,), np.float64)
                have = ci >= 0
                assert np.all(np.isinf(cd[~have])) and (have[:, 0].all() or nc == 1), what
                loc = np.where(have, ci - 1000, 0)
                assert not mask[loc[have]].any(), what
                # exact float64 distances, canonical (distance, index) order
                assert np.array_equal(np.where(have, cd, 0.0), np.where(have, D[np.arange(m)[:, None], loc], 0.0)), what
                key = np.where(have, cd, np.inf)
                ok = (key[:, 1:] > key[:, :-1]) | ((key[:, 1:] == key[:, :-1]) & (loc[:, 1:] > loc[:, :-1])) | ~have[:, 1:]
                assert ok.all(), what
                # the bound: every unmasked reference not emitted lies at squared distance >= bound
                rest = np.where(mask[None, :] == 0, D, np.inf)
                rest[np.arange(m)[:, None], loc] = np.where(have, np.inf, rest[np.arange(m)[:, None], loc])
                nxt = rest.min(1) ** 2
                known = np.isfinite(cb)
                assert known.mean() > 0.95, what
                assert np.all(cb[known] <= nxt[known] * (1 + 1e-12)), what
                assert np.all(cb[known] > 0) and not np.any(cb == np.inf), what
                # the certified entries (d^2 (1 + 1e-12) < bound) are the exact head of the order row
                cert = have & (cd ** 2 * (1 + 1e-12) < cb[:, None])
                assert np.array_equal(np.where(cert, loc, -1), np.where(cert, full_i[:, :nc], -1)), what
                if slack == -1:
                    assert np.array_equal(np.where(have, loc, -1), np.where(have, full_i[:, :nc], -1)), what
            ix.close()


def test_refused_options_leave_the_index_usable(gpu_lib):
    """Unknown names, order_flags (removed) and a split_refs_max that would need more than 1024 / L splits
    are refused (ValueError); after each refusal the same index answers with the oracle's bits."""
    from nabo_amd._synth import pca_like
    n, g, m, k = 5000, 30, 400, 11
    Y, X = pca_like(n, g, seed=91), pca_like(m, g, seed=92)
    want = oracle.knn(X, Y, k, 0, nthreads=16)
    ix = gpu_lib.KnnIndex(n, g, metric=0).set_ref(Y)
    _same(ix.query(X, k), want, "before any refusal")
    with pytest.raises(ValueError):
        ix.set_option("no_such_option", 1)
    _same(ix.query(X, k), want, "after an unknown option")
    with pytest.raises(ValueError, match="builds only"):
        ix.set_option("order_flags", 1)
    _same(ix.query(X, k), want, "after order_flags")
    ix.set_option("split_refs_max", 64)        # one tile per split: 157 splits of 32-entry lists > 1024 / 32
    with pytest.raises(ValueError, match="1024"):
        ix.query(X, k)
    ix.set_option("split_refs_max", 0)
    _same(ix.query(X, k), want, "after a refused split_refs_max")
    ix.close()


if __name__ == "__main__":                       # replay one case: python tests/test_option_sweep_gpu.py metric seed case
    metric, seed, number = (int(a) for a in sys.argv[1:4])
    case = S.cases(metric, seed)[number]
    print(S.describe(case))
    with pytest.MonkeyPatch.context() as mp:
        t = _tally()
        run_case(case, mp, t)
    print("equal to the oracle; rows by pass %s kernels %s" % (dict(t["pass"]), dict(t["kernel"])))
