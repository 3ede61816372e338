"""CPU-side checks of tests/_consumer_refs.py: the plain references agree with the oracle wherever the oracle defines
the operation, the derived bound on the null's mean and sd is met by a float64 two-pass restatement of the kernel on
every case of tests/test_consumers_gpu.py -- and broken by the one-pass formula on the narrow-null case, so that case
can fail -- and the fixed case lists reach every kernel instantiation they claim to."""
import numpy as np
import pytest

import oracle
from oracle import oracle as orc

import _consumer_refs as cr

NULL_CASES = cr.null_cases()


def _oracle_null(c):
    return orc.score_null(c["edge_t"], c["edge_r"], c["w"], c["group"], c["n_ref"], c["n_perm"], seed=c["seed"],
                          score_multiplier=c["multiplier"], key_bits=c["key_bits"])


@pytest.mark.parametrize("name", list(NULL_CASES))
def test_two_pass_float64_meets_the_derived_bound_on_every_null_case(name):
    c = NULL_CASES[name]
    assert c["edge_t"].shape[0] < 5000
    ref = _oracle_null(c)
    mean_ld, sd_ld = cr.null_stats_ld(ref["scores"])
    tol_mean, tol_sd = cr.null_bounds(ref["scores"])
    mean, sd = cr.null_stats_device_order(ref["scores"], two_pass=True)
    assert (np.abs(mean - mean_ld) <= tol_mean).all()
    assert (np.abs(sd - sd_ld) <= tol_sd).all()
    # the oracle's own float64 numpy statistics (pairwise sums, two-pass std) are inside the bound as well
    assert (np.abs(ref["null_mean"] - mean_ld) <= tol_mean).all()
    assert (np.abs(ref["null_sd"] - sd_ld) <= tol_sd).all()
    if c["key_bits"] == 8:
        assert (ref["sizes"] > int(c["group"].sum())).any()              # 8-bit keys tie at the threshold
    if name == "group-all":
        assert (ref["scores"] == ref["obs"][:, None]).all() and (ref["n_ge"] == c["n_perm"]).all()
        assert (sd_ld <= tol_sd).all()


def test_one_pass_variance_breaks_the_bound_on_the_narrow_null():
    """sum(s^2)/P - mean^2, restated in the kernel's summation order: on the node every pooled cell has an equal edge to,
    at multiplier 1e6, the permuted scores differ in their last bits only and the formula returns rounding noise."""
    c = NULL_CASES[cr.NARROW]
    ref = _oracle_null(c)
    _, sd_ld = cr.null_stats_ld(ref["scores"])
    _, tol_sd = cr.null_bounds(ref["scores"])
    _, sd1 = cr.null_stats_device_order(ref["scores"], two_pass=False)
    _, sd2 = cr.null_stats_device_order(ref["scores"], two_pass=True)
    assert 0 < sd_ld[3] < 1e-8 and ref["scores"][3].min() > 1e5           # node 3: a narrow null around ~9e5
    assert abs(sd1[3] - sd_ld[3]) > 1000 * tol_sd[3]
    assert abs(sd2[3] - sd_ld[3]) <= tol_sd[3]


def test_null_cases_reach_every_accumulator_width_and_row_extreme():
    assert {cr.nacc_of(P) for P in cr.NULL_N_PERM} == {1, 2, 4, 8, 17}
    assert {c["key_bits"] for c in NULL_CASES.values()} == set(range(8, 65, 8))
    c = NULL_CASES["rows-mult1e6"]
    deg = np.bincount(c["edge_r"], minlength=c["n_ref"])
    assert deg[0] == 0 and deg[1] == 1 and deg[2] == cr.N_T and deg[3] == cr.N_T
    w2 = c["w"][c["edge_r"] == 2]
    assert w2.min() <= 1e-8 and w2.max() >= 1e8
    assert {c["multiplier"] for c in NULL_CASES.values()} == {1.0, 1000.0, 1e6}
    assert int(NULL_CASES["group-all"]["group"].sum()) == cr.N_T and int(NULL_CASES["group-one"]["group"].sum()) == 1


def test_csr_edge_lists_cover_the_key_widths_and_empty_runs():
    assert cr.CSR_N_REF == [1, 2, 3, 255, 256, 257, 65536, 65537]
    for n_ref in cr.CSR_N_REF:
        lists = cr.csr_edge_lists(n_ref)
        assert ("gap" in lists) == (n_ref > 3000)
        for style, (et, er, w) in lists.items():
            assert er.min() >= 0 and er.max() < n_ref
            order, rp = cr.csr_from_edges(er, n_ref)
            assert rp[0] == 0 and rp[-1] == er.shape[0] and (np.diff(er[order]) >= 0).all()
            if style == "last-node":
                assert (rp[:-1] == 0).all()
            if style == "gap":
                used = np.flatnonzero(np.diff(rp))
                assert used.shape[0] == 2 and used[1] - used[0] > 1000
    n_ref, n_t, et, er, w, group = cr.csr_big_edge_list()
    assert er.shape[0] >= 300000 and (np.bincount(er) >= 50).sum() >= 3


def test_merge_reference_equals_the_oracle_on_sharded_references():
    """the oracle defines the merge through what it must equal: the k-NN over all references"""
    rng = np.random.default_rng(5)
    Y = np.round(rng.standard_normal((90, 3)) * 2)              # a lattice: exact distance ties across shards
    X = np.round(rng.standard_normal((40, 3)) * 2)
    cuts = [0, 17, 18, 60, 90]
    for k, kp, drop in ((5, 6, True), (11, 11, False), (1, 2, True)):
        pi = np.full((4, 40, kp), -1, dtype=np.int64)
        pd = np.full((4, 40, kp), np.inf)
        for s in range(4):
            lo, hi = cuts[s], cuts[s + 1]
            kk = min(kp, hi - lo)
            i, d = oracle.knn(X, Y[lo:hi], kk, 0)
            pi[s, :, :kk], pd[s, :, :kk] = i + lo, d
        gi, gd = cr.merge_ref(pi, pd, k, drop)
        oi, od = oracle.knn(X, Y, k, 0, drop_first=drop)
        assert np.array_equal(gi, oi) and np.array_equal(gd, od)


def test_merge_reference_on_absent_entries_and_short_rows():
    pi = np.array([[[5, -1, -1]], [[-1, -1, -1]], [[cr.MAX_IDX, 2, -1]]], dtype=np.int64)
    pd = np.array([[[1.0, np.inf, np.inf]], [[np.inf] * 3], [[1.0, 3.0, np.inf]]])
    gi, gd = cr.merge_ref(pi, pd, 4, False)
    assert gi.tolist() == [[5, cr.MAX_IDX, 2, -1]] and np.array_equal(gd, [[1.0, 1.0, 3.0, np.nan]], equal_nan=True)
    gi, gd = cr.merge_ref(pi, pd, 3, True)
    assert gi.tolist() == [[cr.MAX_IDX, 2, -1]] and np.array_equal(gd, [[1.0, 3.0, np.nan]], equal_nan=True)


def test_merge_cases_reach_every_width_and_edge():
    assert {cr.merge_width(c[0], c[1]) for c in cr.MERGE_CASES} == {1, 2, 4, 8, 16}
    assert {64, 65, 1024} <= {c[0] * c[1] for c in cr.MERGE_CASES}
    assert {c[2] for c in cr.MERGE_CASES} == {1, 2, 3, 5, 777}
    assert any(c[0] == 1 for c in cr.MERGE_CASES) and any(c[1] == 1 for c in cr.MERGE_CASES)
    for width in (1, 2, 4, 8, 16):
        assert any(cr.merge_width(c[0], c[1]) == width and c[3] + c[4] == c[0] * c[1] for c in cr.MERGE_CASES)
    tied_first = short = near_sentinel = absent_part = 0
    for n_parts, kp, m, k, drop in cr.MERGE_CASES:
        pi, pd = cr.merge_case(n_parts, kp, m, k, drop)
        real = pi >= 0
        assert pi.max() <= cr.MAX_IDX and np.isinf(pd[~real]).all() and np.isfinite(pd[real]).all()
        for row in range(m):
            v = pi[:, row][real[:, row]]
            assert np.unique(v).shape[0] == v.shape[0]                    # global indices are distinct within a row
            for p in range(n_parts):                                      # every part row is in the canonical order
                n = int(real[p, row].sum())
                assert real[p, row, :n].all()
                o = np.lexsort((pi[p, row, :n], pd[p, row, :n]))
                assert np.array_equal(o, np.arange(n))
        d0 = np.sort(pd[:, 0][real[:, 0]])
        tied_first += int(d0.shape[0] > 1 and d0[0] == d0[1] and bool(drop))
        short += int((real.sum(axis=(0, 2)) < k + drop).any())
        near_sentinel += int((pi == cr.MAX_IDX).any())
        absent_part += int((~real).all(axis=2).any())
    assert tied_first >= 3 and short >= 8 and near_sentinel >= 10 and absent_part >= 8


def test_snn_reference_equals_the_oracle_where_no_entry_is_absent():
    for m, n, k in cr.SNN_SHAPES:
        t_idx, r_idx = cr.snn_case(m, n, k)
        assert all(np.unique(r).shape[0] == k for r in t_idx) and all(np.unique(r).shape[0] == k for r in r_idx)
        cnt = cr.snn_ref(t_idx, r_idx, k)
        assert cnt.max() >= (1 if k == 1 else 2)                          # the cases do share neighbours
        ot, oj, os_ = _oracle_counts(t_idx, r_idx, k)
        tt, ss = np.nonzero(cnt > 0)
        assert np.array_equal(tt, ot) and np.array_equal(t_idx[tt, ss], oj) and np.array_equal(cnt[tt, ss], os_)


def _oracle_counts(t_idx, r_idx, k):
    m = t_idx.shape[0]
    ot, oj, os_ = np.empty(m * k, dtype=np.int64), np.empty(m * k, dtype=np.int64), np.empty(m * k, dtype=np.int32)
    ne = orc.lib().oracle_snn_counts(np.ascontiguousarray(t_idx), m, np.ascontiguousarray(r_idx), r_idx.shape[0], k,
                                     ot, oj, os_)
    return ot[:ne], oj[:ne], os_[:ne]


def test_snn_reference_never_counts_absent_entries():
    t_idx = np.array([[0, 2, -1, -1], [1, -1, -1, -1], [3, 0, 1, 9]], dtype=np.int64)
    r_idx = np.array([[0, 2, 1, -1], [-1, -1, -1, -1], [2, 0, -1, -1], [3, 1, 0, 2]], dtype=np.int64)
    assert cr.snn_ref(t_idx, r_idx, 4).tolist() == [[2, 2, 0, 0], [0, 0, 0, 0], [3, 2, 0, 0]]
    for m, n, k in cr.SNN_SHAPES:
        for absent in cr.SNN_ABSENT[1:]:
            t_idx, r_idx = cr.snn_case(m, n, k, absent)
            assert (t_idx < 0).any() or (r_idx < 0).any()
            cnt = cr.snn_ref(t_idx, r_idx, k)
            real_t = (t_idx >= 0).sum(axis=1)
            assert (cnt <= real_t[:, None]).all() and (cnt[(t_idx < 0) | (t_idx >= n)] == 0).all()
