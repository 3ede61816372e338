"""The kernels that CONSUME the k-NN lists, at their edges, against plain references (tests/_consumer_refs.py):
the permutation null (null_hist / null_label / null_score_kernel<NACC>, score_null.hip), the device CSR build
(csr_build.hip), the shard merge (merge_kernel<NCL, true> behind nabo_merge_topk), the SNN counts (snn_counts_kernel)
and the literal pairwise kernel at the ends of its grid.  Every case is fixed and seeded.

Which case runs which instantiation:
  null_score_kernel<1>  n_perm 1 .. 255      <2>  256 .. 511 (256, 257, 300)     <4>  1023
                    <8>  1024, 2047          <17> 2048, 4095, 4096
  merge_kernel<1, true>  n_parts*kp = 1, 21, 64    <2>  65, 128    <4>  168, 256    <8>  288, 512    <16> 544, 1024
"""
import ctypes as C

import numpy as np
import pytest

import oracle
from oracle import oracle as orc

import _consumer_refs as cr

pytestmark = pytest.mark.gpu
NULL_CASES = cr.null_cases()


# ---- 1. permutation null ----------------------------------------------------------------------------------------------
def _null_edges(c, n_ref=None, edge_r=None, edge_t=None):
    """nabo_score_null_edges through the package (the edge list as the caller has it)"""
    import nabo_amd
    return nabo_amd.mapping_score_null(c["edge_t"] if edge_t is None else edge_t, c["edge_r"] if edge_r is None else edge_r,
                                       c["w"], c["group"], c["n_ref"] if n_ref is None else n_ref, n_perm=c["n_perm"],
                                       seed=c["seed"], score_multiplier=c["multiplier"], key_bits=c["key_bits"])


def _null_csr(c):
    """nabo_score_null on the CSR a stable host sort of the same edge list gives"""
    from nabo_amd import _lib
    n_ref, P = c["n_ref"], c["n_perm"]
    order, rp = cr.csr_from_edges(c["edge_r"], n_ref)
    et = np.ascontiguousarray(np.asarray(c["edge_t"])[order], dtype=np.int64)
    ew = np.ascontiguousarray(np.asarray(c["w"])[order], dtype=np.float64)
    grp = np.ascontiguousarray(np.asarray(c["group"]) != 0, dtype=np.uint8)
    obs, mean, sd = np.empty(n_ref), np.empty(n_ref), np.empty(n_ref)
    nge, sizes = np.empty(n_ref, dtype=np.int64), np.empty(P, dtype=np.int64)
    L = _lib.lib()
    L.nabo_score_null.argtypes = [C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                  C.c_int32, C.c_uint64, C.c_int32, C.c_double] + [C.c_void_p] * 5
    _lib.check(L.nabo_score_null(0, n_ref, rp.ctypes.data, et.ctypes.data, ew.ctypes.data, grp.shape[0], grp.ctypes.data,
                                 P, int(c["seed"]), int(c["key_bits"]), float(c["multiplier"]), obs.ctypes.data,
                                 nge.ctypes.data, mean.ctypes.data, sd.ctypes.data, sizes.ctypes.data))
    return {"obs": obs, "n_ge": nge, "null_mean": mean, "null_sd": sd, "sizes": sizes}


def _same_bits(a, b):
    for key in ("obs", "n_ge", "null_mean", "null_sd", "sizes"):
        assert np.array_equal(a[key], b[key]), key


@pytest.mark.parametrize("name", list(NULL_CASES))
def test_null_vs_oracle(gpu_lib, name):
    """sizes, obs and n_ge bit-equal to the oracle; mean and sd within the derived bound (_consumer_refs.null_bounds) of
    the two-pass longdouble statistics of the oracle's score matrix; both entry points give the same bits."""
    c = NULL_CASES[name]
    ref = orc.score_null(c["edge_t"], c["edge_r"], c["w"], c["group"], c["n_ref"], c["n_perm"], seed=c["seed"],
                         score_multiplier=c["multiplier"], key_bits=c["key_bits"])
    res = _null_edges(c)
    assert np.array_equal(res["sizes"], ref["sizes"])
    assert np.array_equal(res["obs"], ref["obs"])
    assert np.array_equal(res["n_ge"], ref["n_ge"])
    mean_ld, sd_ld = cr.null_stats_ld(ref["scores"])
    tol_mean, tol_sd = cr.null_bounds(ref["scores"])
    err_mean, err_sd = np.abs(res["null_mean"] - mean_ld), np.abs(res["null_sd"] - sd_ld)
    print("%s: max |mean-ref| / bound = %.3g, max |sd-ref| / bound = %.3g, worst sd %.6g against %.6g" % (
        name, float((err_mean / np.maximum(tol_mean, 1e-300)).max()), float((err_sd / np.maximum(tol_sd, 1e-300)).max()),
        float(res["null_sd"][np.argmax(err_sd)]), float(sd_ld[np.argmax(err_sd)])))
    assert (err_mean <= tol_mean).all()
    assert (err_sd <= tol_sd).all()
    _same_bits(_null_csr(c), res)
    n_a = int(np.asarray(c["group"]).sum())
    if c["key_bits"] == 8:
        assert (res["sizes"] > n_a).any()                                # 8-bit keys tie at the threshold
    if c["key_bits"] >= 32:
        assert (res["sizes"] == n_a).all()
    if name == "group-all":                                              # every permutation labels every cell
        assert (res["n_ge"] == c["n_perm"]).all()
    if name.startswith("rows-"):
        assert res["obs"][0] == 0.0 and res["n_ge"][0] == c["n_perm"] and res["null_sd"][0] == 0.0      # no edge at all


@pytest.mark.parametrize("n_ref", cr.CSR_N_REF)
def test_null_edge_list_equals_csr_at_every_key_width(gpu_lib, n_ref):
    """csr_keys / rocPRIM sort over key_bits_for(n_ref) bits / csr_rowptr / csr_gather: the edge-list entry point equals
    the CSR entry point fed a host np.argsort(kind="stable"), bit for bit (mean and sd included)."""
    n_t = 500
    rng = np.random.default_rng(n_ref)
    group = (rng.random(n_t) < 0.4).astype(np.uint8)
    group[0] = 1
    for style, (et, er, w) in cr.csr_edge_lists(n_ref, n_t).items():
        c = {"edge_t": et, "edge_r": er, "w": w, "group": group, "n_ref": n_ref, "n_perm": 33, "seed": 5 + n_ref,
             "multiplier": 1000.0, "key_bits": 64}
        res = _null_edges(c)
        _same_bits(_null_csr(c), res)
        used = np.bincount(er, minlength=n_ref) > 0
        assert not res["obs"][~used].any() and (res["n_ge"][~used] == 33).all(), style       # empty rows score 0
        assert res["obs"][used].any(), style


def test_null_edge_list_of_several_sort_blocks(gpu_lib):
    n_ref, n_t, et, er, w, group = cr.csr_big_edge_list()
    c = {"edge_t": et, "edge_r": er, "w": w, "group": group, "n_ref": n_ref, "n_perm": 64, "seed": 99,
         "multiplier": 1000.0, "key_bits": 64}
    res = _null_edges(c)
    _same_bits(_null_csr(c), res)
    # the observed score is a plain segmented sum: in the caller's order per row, in float64
    order, rp = cr.csr_from_edges(er, n_ref)
    keep = group[et[order]] != 0
    for r in (0, 4095, 4096, 65535, 65536, n_ref - 1):
        acc = 0.0
        for e in range(rp[r], rp[r + 1]):
            acc = acc + (w[order[e]] if keep[e] else 0.0)
        assert res["obs"][r] == (1000.0 * acc) / float(group.sum())


def test_null_edge_list_refuses_an_index_out_of_range_at_the_last_edge(gpu_lib):
    c = dict(NULL_CASES["nperm-33"])
    for bad in (c["n_ref"], -1):
        er = c["edge_r"].copy()
        er[-1] = bad
        with pytest.raises(ValueError):
            _null_edges(c, edge_r=er)
    for bad in (cr.N_T, -1):
        et = c["edge_t"].copy()
        et[-1] = bad
        with pytest.raises(ValueError):
            _null_edges(c, edge_t=et)
    _same_bits(_null_csr(c), _null_edges(c))                             # and the device goes on working


# ---- 2. shard merge ---------------------------------------------------------------------------------------------------
def _merge(pi, pd, k, drop):
    from nabo_amd import _knn
    n_parts, m, kp = pi.shape
    dpi = _knn.DeviceBuffer(pi.nbytes).upload(pi)
    dpd = _knn.DeviceBuffer(pd.nbytes).upload(pd)
    doi, dod = _knn.DeviceBuffer(m * k * 8), _knn.DeviceBuffer(m * k * 8)
    try:
        _knn.merge_topk_device(dpi.ptr, dpd.ptr, n_parts, m, kp, k, drop, doi.ptr, dod.ptr)
        return doi.download((m, k), np.int64), dod.download((m, k), np.float64)
    finally:
        for b in (dpi, dpd, doi, dod):
            b.free()


@pytest.mark.parametrize("n_parts,kp,m,k,drop", cr.MERGE_CASES)
def test_merge_topk_vs_reference(gpu_lib, n_parts, kp, m, k, drop):
    pi, pd = cr.merge_case(n_parts, kp, m, k, drop)
    gi, gd = _merge(pi, pd, k, drop)
    ri, rd = cr.merge_ref(pi, pd, k, drop)
    assert np.array_equal(gi, ri), "indices differ in rows %s" % np.flatnonzero((gi != ri).any(axis=1))[:8]
    assert np.array_equal(gd, rd, equal_nan=True)
    assert np.isnan(gd[gi < 0]).all() and np.isfinite(gd[gi >= 0]).all()


def test_merge_topk_copied_distances_order_by_global_index(gpu_lib):
    """one part's distances copied into the others under different indices: every distance is tied n_parts times"""
    rng = np.random.default_rng(8)
    n_parts, m, kp, k = 5, 5, 20, 40
    d = np.sort(rng.random((m, kp)), axis=1)
    pd = np.ascontiguousarray(np.broadcast_to(d, (n_parts, m, kp)))
    base = np.array([3000000000, 7, cr.MAX_IDX - 100, 1 << 31, 100000], dtype=np.int64)
    pi = np.ascontiguousarray(base[:, None, None] + np.arange(kp, dtype=np.int64)[None, None, :] +
                              np.zeros((1, m, 1), dtype=np.int64))
    for drop in (False, True):
        gi, gd = _merge(pi, pd, k, drop)
        ri, rd = cr.merge_ref(pi, pd, k, drop)
        assert np.array_equal(gi, ri) and np.array_equal(gd, rd)


def test_merge_topk_refusals_leave_the_device_usable(gpu_lib):
    pi, pd = cr.merge_case(3, 7, 5, 11, True)
    big_i, big_d = np.full((33, 2, 32), -1, dtype=np.int64), np.full((33, 2, 32), np.inf)
    with pytest.raises(ValueError):
        _merge(big_i, big_d, 5, False)                                   # n_parts * kp = 1056 > 1024
    with pytest.raises(ValueError):
        _merge(pi, pd, 21, True)                                         # k + drop = 22 > 21
    with pytest.raises(ValueError):
        _merge(pi, pd, 22, False)
    gi, gd = _merge(pi, pd, 11, True)
    ri, rd = cr.merge_ref(pi, pd, 11, True)
    assert np.array_equal(gi, ri) and np.array_equal(gd, rd, equal_nan=True)


# ---- 3. SNN counts ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("absent", cr.SNN_ABSENT)
@pytest.mark.parametrize("m,n,k", cr.SNN_SHAPES)
def test_snn_counts_vs_python_sets(gpu_lib, m, n, k, absent):
    """target <-> reference form (m != n); rows ending in 1 .. k absent (-1) entries in t_idx, r_idx or both never count
    (include/nabo_knn.h: entries < 0 belong to neither set); a slot whose entry is absent or >= n is 0."""
    t_idx, r_idx = cr.snn_case(m, n, k, absent)
    cnt = gpu_lib.snn_counts(t_idx, r_idx, k)
    ref = cr.snn_ref(t_idx, r_idx, k)
    bad = np.flatnonzero((cnt != ref).any(axis=1))
    assert bad.size == 0, "%d rows differ, first %d: got %s expected %s" % (bad.size, bad[0], cnt[bad[0]], ref[bad[0]])


def test_snn_edges_with_absent_entries(gpu_lib):
    """Mapping-level consequence: the edge list of rows that end in absent entries holds exactly the (t, j) pairs whose
    SETS intersect, weighted by the size of that intersection, a cell's edges in the order set(its real entries)
    iterates."""
    from nabo_amd import _mapping
    m, n, k = 257, 1000, 11
    t_idx, r_idx = cr.snn_case(m, n, k, "both")
    tt, jj, w = _mapping.snn_edges(t_idx, r_idx, k)
    ref = cr.snn_ref(t_idx, r_idx, k)
    exp = []
    for t in range(m):
        real = [int(v) for v in t_idx[t] if v >= 0]
        slot = {v: s for s, v in enumerate(t_idx[t].tolist())}
        for j in set(real):                                              # the interpreter's own iteration order
            if ref[t, slot[j]] > 0:
                exp.append((t, j, oracle.snn_weight(int(ref[t, slot[j]]), k)))
    assert len(exp) > m and (t_idx < 0).any()
    assert list(zip(tt.tolist(), jj.tolist(), w.tolist())) == exp


# ---- 4. pairwise at the ends of its grid ------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [0, 1, 2])
@pytest.mark.parametrize("g", [1, 50])
@pytest.mark.parametrize("m,n", [(65535, 1), (3, 70001)])
def test_pairwise_grid_edges_vs_oracle(gpu_lib, m, n, g, metric):
    """m = 65535 is the documented last row count (grid.y); n = 70001 is 274 blocks in x with m > 1"""
    from nabo_amd._synth import pca_like
    X, Y = pca_like(m, g, seed=600 + g), pca_like(n, g, seed=700 + g)
    D = gpu_lib.pairwise(X, Y, metric, 0.25)
    assert np.array_equal(D, oracle.pairwise(X, Y, metric, 0.25, nthreads=8))


def test_pairwise_refuses_more_rows_than_one_launch_holds(gpu_lib):
    X, Y = np.zeros((65536, 2)), np.ones((1, 2))
    with pytest.raises(ValueError):
        gpu_lib.pairwise(X, Y, 0)
    assert np.array_equal(gpu_lib.pairwise(X[:5], Y, 0), np.full((5, 1), np.sqrt(2.0)))
