"""tests/_refine_ref.py (the restatement tests/test_refine_gpu.py holds refine.hip to) on the CPU: rows worked by hand, two
per branch of the verdict, and every case of the GPU test built and inspected:

  * no row's deciding comparison lies within 1e-9 (relative) of equality unless it is a comparison of exactly
    representable values (margin 0), so the GPU test demands equal verdicts everywhere and excuses nothing.  1e-9 is far
    above the float64 rounding of the ten operations of the certificate (~1e-15) and far below E / d_k'^2 (~1e-5);
  * per metric and per (S, L) shape the cases reach every branch;
  * the lists are sound (every valid reference outside a list scores >= the list's threshold).

Hand numbers (Euclidean): ||x||^2 = 4, max ||y|| = 2, err_coef = 2^-10: E = 2^-10 * 16 = 2^-6; tau = 64 in score units of
2^-6: bound = (1 + 4 - 0.015625)(1 - 1e-12) = 4.984375 (1 - 1e-12).  Cosine: ||x^||^2 = 1, max ||y^|| = 1, E = 2^-8,
tau = 32: bound = 1.49609375 (1 - 1e-12), certificate value 0.748046875 (1 - 1e-12) - 2e-13.
"""
import math

import numpy as np
import pytest

import oracle

import _refine_ref as rr

F32 = np.float32
INF32 = F32(np.inf)
PAD = rr.PAD


def _v(metric, nreal, kk, dk, taus, n_valid=10 ** 6, ie=0, last=(PAD,), xn=4.0, err_coef=2.0 ** -10, ymax=2.0, g=7,
       plateau=F32(0.0)):
    return rr.verdict(metric, nreal, kk, dk, ie, np.asarray(taus, dtype=F32), last, n_valid, xn, err_coef, ymax, 2.0 ** -6, g,
                      plateau)


def test_verdict_by_hand_counts_and_infinite_thresholds():
    assert _v(0, 3, 5, None, [INF32], n_valid=3) == (True, "short_ok", 0.0)
    assert _v(0, 3, 5, None, [64.0], n_valid=4) == (False, "short_fail", 0.0)
    assert _v(1, 0, 1, None, [INF32], n_valid=0) == (True, "short_ok", 0.0)
    assert _v(2, 4, 5, None, [INF32], n_valid=9) == (False, "short_fail", 0.0)
    assert _v(0, 5, 5, 2.0, [INF32, INF32], n_valid=5) == (True, "inf_ok", 0.0)
    assert _v(0, 5, 5, 2.0, [INF32, INF32], n_valid=6) == (False, "inf_fail", 0.0)
    assert _v(1, 9, 5, 2.0, [INF32], n_valid=9)[:2] == (True, "inf_ok")
    assert _v(2, 9, 5, 0.1, [INF32], n_valid=10)[:2] == (False, "inf_fail")


def test_verdict_by_hand_euclidean_and_cosine():
    ok, br, mg = _v(0, 9, 5, 2.0, [64.0, 80.0, INF32])                    # 4.984375 > 4
    assert (ok, br) == (True, "cert") and mg == pytest.approx(0.984375 / 4.984375, rel=1e-9)
    assert _v(0, 9, 5, 2.25, [80.0, 64.0])[:2] == (False, "fail")         # 5.0625
    d = math.sqrt(4.99)                                                  # between bound and bound + E: E alone fails it
    assert _v(0, 9, 5, d, [64.0])[:2] == (False, "fail")
    assert _v(0, 9, 5, d, [64.0], err_coef=0.0)[:2] == (True, "cert")
    # tau_scale counts: the same threshold read as 64 * 1 would certify anything here
    assert _v(0, 9, 5, 2.2, [64.0])[:2] == (True, "cert") and _v(0, 9, 5, 2.3, [64.0])[:2] == (False, "fail")
    # the two 1e-12 factors: bound == d^2 exactly does not certify
    assert _v(0, 9, 5, math.sqrt(4.984375), [64.0])[0] is False
    kw = dict(xn=1.0, ymax=1.0)
    assert _v(2, 9, 5, 0.5, [32.0], **kw)[:2] == (True, "cert")            # 0.748 > 0.5
    assert _v(2, 9, 5, 0.75, [32.0], **kw)[:2] == (False, "fail")
    assert _v(2, 9, 5, 0.748046875, [32.0], **kw)[0] is False              # the 2e-13
    assert _v(2, 9, 5, 0.749, [32.0], err_coef=0.0, **kw)[0] is True and _v(2, 9, 5, 0.749, [32.0], **kw)[0] is False


def test_verdict_by_hand_canberra():
    _, pl = rr.cb_constants(7)
    assert pl == F32(7.0) - F32(63.0 * 2.0 ** -24) and pl < F32(7.0)
    assert _v(1, 9, 5, 2.0, [2.0, 3.0], plateau=pl) == (False, "fail", 0.0)             # tau == d_k'
    assert _v(1, 9, 5, 2.0, [np.nextafter(F32(2.0), INF32)], plateau=pl)[:2] == (True, "cert")
    assert _v(1, 9, 5, 1.0, [pl, pl], plateau=pl)[:2] == (True, "plateau_near")
    assert _v(1, 9, 5, 6.25, [pl], plateau=pl)[:2] == (True, "plateau_near")
    assert _v(1, 9, 5, 7.0, [pl, pl], ie=31, last=(31, 40), plateau=pl) == (True, "plateau_le", 0.0)
    assert _v(1, 9, 5, 7.0, [pl, pl], ie=32, last=(31, 40), plateau=pl) == (False, "plateau_gt", 0.0)
    # only the lists AT the plateau count, and it is the list's last entry (not its smallest)
    assert _v(1, 9, 5, 7.0, [pl, INF32], ie=35, last=(40, 31), plateau=pl)[1] == "plateau_le"
    assert _v(1, 9, 5, 7.0, [pl, pl, F32(6.5)], ie=0, last=(31, 40, 50), plateau=pl)[:2] == (False, "fail")


def test_refine_rows_by_hand():
    # g = 1: target 0 at row 1 (row0 = 1), references 3, 1, 2, 1 (a duplicate), 10 (masked); k = 2, drop = 1
    X = np.array([[9.0], [0.0]])
    Y = np.array([[3.0], [1.0], [2.0], [1.0], [10.0]])
    cand = np.array([[0, 3, PAD, PAD, 2, 1, PAD, PAD]], dtype=np.uint32)
    out = rr.refine(X, 1, 2, Y, 1, cand, np.array([[INF32, INF32]]), 2, 4, np.array([81.0, 0.0]), 0.0, 10.0, 1.0, 2, 1, 100, 4,
                    np.array([4], dtype=np.uint32), 1, 0)
    assert out.branch == ["inf_ok"] and out.idx.tolist() == [[103, 102]] and out.dist.tolist() == [[1.0, 2.0]]
    # k' = 6 > 4 candidates: the masked tail, then -1 / NaN
    out = rr.refine(X, 1, 2, Y, 1, cand, np.array([[INF32, INF32]]), 2, 4, np.array([81.0, 0.0]), 0.0, 10.0, 1.0, 5, 1, 100, 4,
                    np.array([4], dtype=np.uint32), 1, 0)
    assert out.branch == ["short_ok"] and out.idx.tolist() == [[103, 102, 100, 104, -1]]
    assert out.dist[0, :4].tolist() == [1.0, 2.0, 3.0, 10.0] and np.isnan(out.dist[0, 4])
    # a threshold of 3 in scores a = d^2 - 0: bound 3 (1 - 1e-12) < d_3^2 = 4: fails; its seed is the first float32 above 4
    out = rr.refine(X, 1, 2, Y, 1, cand, np.array([[INF32, F32(3.0)]]), 2, 4, np.array([81.0, 0.0]), 0.0, 10.0, 1.0, 2, 1, 100, 4,
                    np.array([4], dtype=np.uint32), 1, 0)
    assert out.branch == ["fail"] and out.seed_lo[0] == np.nextafter(F32(4.0), INF32)
    assert rr.lower_seed(out.seed_lo[0], 2.0, 1.0) < F32(4.0)


def test_refine_cand_by_hand():
    X = np.array([[0.0], [0.0], [0.0]])
    Y = np.array([[3.0], [1.0], [2.0], [1.0]])
    cand = np.array([[0, 3, 2, 1]] * 3, dtype=np.uint32)
    tau = np.array([[INF32], [F32(20.0)], [INF32]])
    xn = np.array([0.0, 0.0, np.nan])
    idx, dist, bound = rr.refine_cand(X, 0, 3, Y, 1, cand, tau, 1, 4, xn, 0.0, 10.0, 1.0, 2, 10, 4, 0)
    assert idx.tolist() == [[11, 13]] * 3 and dist.tolist() == [[1.0, 1.0]] * 3
    assert bound.tolist() == [4.0 * (1.0 - 1e-12), 4.0 * (1.0 - 1e-12), -np.inf]      # d_(kout) = 2 decides
    idx, dist, bound = rr.refine_cand(X, 0, 3, Y, 1, cand, tau, 1, 4, xn, 0.0, 10.0, 1.0, 6, 10, 4, 0)
    assert idx[0].tolist() == [11, 13, 12, 10, -1, -1] and dist[0, 4:].tolist() == [np.inf, np.inf]
    assert bound.tolist() == [np.inf, 20.0 * (1.0 - 1e-12), -np.inf]
    _, _, bound = rr.refine_cand(X, 0, 3, Y, 1, cand, tau, 1, 4, xn, 0.0, 10.0, 1.0, 6, 10, 5, 0)
    assert bound.tolist() == [-np.inf, 20.0 * (1.0 - 1e-12), -np.inf]                 # a reference is missing, nothing dropped


def test_merge_lists_by_hand():
    idx = np.array([[5, 9, PAD, 2, 7, 8]], dtype=np.uint32)
    key = np.array([[1.0, 4.0, 99.0, -2.0, 4.0, 6.0]], dtype=F32)
    tau = np.array([[5.0, 6.5]], dtype=F32)
    oi, ot = rr.merge_lists(idx, key, tau, 1, 2, 3, 3, 4)
    assert oi.tolist() == [[2, 5, 7, PAD]] and ot.tolist() == [4.0]          # (4.0, 7) before (4.0, 9); 9's key is the cut
    oi, ot = rr.merge_lists(idx, key, tau, 1, 2, 3, 4, 4)
    assert oi.tolist() == [[2, 5, 7, 9]] and ot.tolist() == [5.0]            # the cut (6.0) is above list 0's tau
    oi, ot = rr.merge_lists(idx, key, tau, 1, 2, 3, 5, 8)
    assert oi.tolist() == [[2, 5, 7, 9, 8, PAD, PAD, PAD]] and ot.tolist() == [5.0]


def test_exact_rows_tail_and_normalise():
    rng = np.random.default_rng(5)
    X, Y = rng.standard_normal((6, 5)), rng.standard_normal((40, 5))
    Y[20] = Y[3]
    mask = (rng.random(40) < 0.3).astype(np.uint8)
    ml = np.flatnonzero(mask).astype(np.uint32)
    rows = np.array([4, 1, 5], dtype=np.uint32)
    for metric in (0, 1, 2):
        for k, drop in ((7, 0), (7, 1), (35, 1)):                   # 35 + 1 > the valid references: the masked ones follow
            ei, ed = oracle.knn(X[rows], Y, k, metric=metric, ref_mask=mask, drop_first=bool(drop))
            gi, gd = rr.exact_rows(X, Y, 40, 5, metric, 0.25, mask, rows, 3, k, drop, 1000, ml, ml.shape[0])
            assert np.array_equal(gi, ei + 1000) and np.array_equal(gd.view(np.uint64), ed.view(np.uint64))
    gi, gd = rr.exact_rows(X, Y, 40, 5, 0, 0.25, mask, rows, 3, 38, 0, 0, ml, 2)      # the list is shorter than the gap
    nv = 40 - ml.shape[0]
    assert gi[:, nv:nv + 2].tolist() == [ml[:2].tolist()] * 3 and (gi[:, nv + 2:] == -1).all() and np.isnan(gd[:, nv + 2:]).all()
    ti, td, wr = rr.masked_tail(X, 6, Y, 5, 0, 0.25, ml, 2, 3, 7, 1, 50)
    assert wr.tolist() == [False, False, True, True, True, True, True]
    assert ti[2].tolist() == [-7, -7, 50 + ml[0], 50 + ml[1], -1, -1, -1] and td[2, 2] == oracle.pairwise(X[2:3], Y[ml[:1]])[0, 0]
    N = rr.normalise_rows(np.array([[3.0, 4.0], [0.0, 0.0], [0.0, -2.0]]))
    assert N.tolist() == [[0.6, 0.8], [0.0, 0.0], [0.0, -1.0]]


def test_canberra_exact_case_is_what_it_says():
    c = rr.canberra_exact_case()
    out = rr.run_refine(c)
    assert [(bool(a), b) for a, b in zip(out.certified, out.branch)] == c.expect
    assert out.margin[0] == 0.0 and out.dk[0] == 2.0 and c.cand_tau[0].min() == F32(2.0)
    assert out.dk[2] == out.dk[3] == out.dk[5] == out.dk[6] == 7.0
    assert c.cand_idx[6, 31] == 1 and c.cand_idx[3, 31] == 0 and c.cand_idx[2, 31] == 31      # list 0's last entry: pmin


NEED_L2 = ["comfortable", "e_only", "hair_fail", "hair_cert", "short_ok", "short_fail", "inf_ok", "inf_fail", "tie", "dup_in"]
NEED_CB = ["comfortable", "hair_fail", "hair_cert", "short_ok", "short_fail", "inf_ok", "inf_fail", "tie", "dup_in",
           "plateau_near", "plateau_le", "plateau_gt"]


@pytest.mark.parametrize("metric", [0, 1, 2])
def test_cases_keep_their_margin_and_reach_every_branch(metric):
    counts = {sh: dict.fromkeys(NEED_CB if metric == 1 else NEED_L2, 0) for sh in rr.SHAPES}
    for name in rr.case_names():
        c = rr.make_case(name, metric)
        rows = c.m - c.row0
        assert rows % 4 != 0 and c.cand_idx.shape == (rows, c.S * c.L)
        real = c.cand_idx[c.cand_idx != PAD]
        assert real.size == 0 or (real.max() < c.n and not c.mask[real].any()), name     # nothing out of range, nothing masked
        out = rr.run_refine(c)
        noE = rr.run_refine(c, err_coef=0.0, want_seed=False) if metric != 1 else None
        chunk = (c.n + c.S - 1) // c.S
        cnt = counts[(c.S, c.L)]
        for r in range(rows):
            what = "%s metric %d row %d (%s, %s)" % (name, metric, r, c.kind[r], out.branch[r])
            assert out.margin[r] == 0.0 or out.margin[r] >= rr.MARGIN, "%s: margin %.3g" % (what, out.margin[r])
            if c.kind[r] != "vanished":                     # sound lists: what is not a candidate scores >= its split's tau
                ci = c.cand_idx[r][c.cand_idx[r] != PAD]
                outside = np.setdiff1d(np.flatnonzero(c.mask == 0), ci)
                assert (c.key[r, outside] >= c.cand_tau[r, outside // chunk]).all(), what
            kd, br, ok = c.kind[r], out.branch[r], bool(out.certified[r])
            if kd == "plain" and br == "cert" and out.margin[r] >= 1e-4:
                cnt["comfortable"] += 1
            elif kd == "e_only":
                assert not ok and noE.certified[r], what
                cnt[kd] += 1
            elif kd in ("hair_fail", "hair_cert"):
                assert ok == (kd == "hair_cert") and br in ("cert", "fail") and out.margin[r] < 1e-3, what
                cnt[kd] += 1
            elif kd == "tie":
                assert not ok and br == "fail", what
                cnt[kd] += 1
            elif kd == "dup_in":
                assert ok, what
                cnt[kd] += 1
            elif kd.startswith("plateau"):
                assert br == kd and (kd == "plateau_near" or out.dk[r] == float(c.g)), what
                cnt[kd] += 1
            elif br in ("short_ok", "short_fail", "inf_ok", "inf_fail"):
                assert (kd == "vanished") == (not ok), what
                cnt[br] += 1
            if br == "fail" and metric != 1:                # the seed interval is not empty and does what it says
                T = out.seed_lo[r]
                assert np.isfinite(T) and rr.lower_seed(T, out.dk[r], c.tau_scale) < T, what
    for sh, cnt in counts.items():
        assert all(v > 0 for v in cnt.values()), "metric %d shape %s: %s" % (metric, sh, cnt)


@pytest.mark.parametrize("metric", [0, 2])
def test_merged_cases_keep_their_margin(metric):
    """tests/test_refine_gpu.py also refines the MERGED lists of these cases (the product's sequence): same condition"""
    for name in ["main8", "main9", "main10", "main11", "main12"]:
        c = rr.make_case(name, metric)
        rows = c.m - c.row0
        lkeep, Lout = rr.merged_shape(c)
        mi, mt = rr.merge_lists(c.cand_idx, c.cand_key, c.cand_tau, rows, c.S, c.L, lkeep, Lout)
        out = rr.run_refine(c, cand_idx=mi, cand_tau=mt.reshape(rows, 1), S=1, L=Lout, want_seed=False)
        plain = rr.run_refine(c, want_seed=False)
        assert ((out.margin == 0.0) | (out.margin >= rr.MARGIN)).all(), (name, out.margin[(out.margin != 0) & (out.margin < rr.MARGIN)])
        assert not (out.certified & ~plain.certified).any(), name
