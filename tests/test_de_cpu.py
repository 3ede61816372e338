"""The Mann-Whitney DE test and cluster markers (include/nabo_de.h, nabo_amd/_de.py) without a GPU: the C header and its
symbols, argument checks, the no-device failure, the tests' plain restatement against the reference's tables
(tests/golden/de.npz, tools/gen_golden_de.py), and the host logic -- carry-over of an empty group, Benjamini-Hochberg,
ordering, filtering, marker counting -- with the device step replaced by that restatement.  Then the edge cases of
tests/_de_edges.py: the restatement against the dense reference (tests/_de_dense_ref.py), and the library's exact p
(nabo_amd/csrc/de_exact.h, compiled for the host) against Python integers."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import nabo_amd
from nabo_amd import _de, _lib

import _de_dense_ref as dense
import _de_edges as edges
import _de_ref as dref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ULP = 2.0 ** -52


def tolerances(d):
    """log2_fc: 4 x the measured float32-vs-float64 deviation of the reference's own value (the orders of the float64
    sums differ by some 2^-29 of that).  pval, qval: the measured deviation of the reference's p from math.erfc plus
    2 ulp -- p is computed on the host side of the ABI with libm's erfc from a z that is bit-equal to the
    restatement's, because no error bound of the device library's double erfc could be quoted."""
    return 4 * float(d["log2fc_dev"]), float(d["p_dev"]) + 2 * ULP


def build_de_check(tmp_path):
    exe = os.path.join(str(tmp_path), "de_check")
    cmd = ["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(REPO, "include"),
           os.path.join(REPO, "tests", "abi_c", "de_check.c"), "-L" + os.path.join(REPO, "nabo_amd"), "-lnabo_knn",
           "-Wl,-rpath," + os.path.join(REPO, "nabo_amd"), "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0, r.stdout
    return exe


def test_header_is_plain_c_and_links(tmp_path):
    _lib.lib()
    exe = build_de_check(tmp_path)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0 and "%d entry points" % len(_lib.DE_SYMBOLS) in r.stdout, r.stdout


def test_library_exports_de_symbols():
    src = open(os.path.join(REPO, "include", "nabo_de.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = sorted(set(re.findall(r"\b(nabo_[a-z0-9_]+)\s*\(", src)))
    assert declared == sorted(_lib.DE_SYMBOLS)
    assert not set(_lib.DE_SYMBOLS) & (set(_lib.SYMBOLS) | set(_lib.GRAPH_SYMBOLS) | set(_lib.CLUSTER_SYMBOLS))
    L = _lib.lib()
    for n in _lib.DE_SYMBOLS:
        assert hasattr(L, n), n


def test_public_names():
    for n in ("de_test_csc", "run_de_test", "find_cluster_markers"):
        assert n in nabo_amd.__all__ and callable(getattr(nabo_amd, n))


GOOD = dict(gene_ptr=[0, 2, 3], cell=[0, 2, 1], val=[1.0, 2.0, 3.0], sf=[1.0, 1.0, 1.0], set_ptr=[0, 2, 3], members=[0, 1, 2])


@pytest.mark.parametrize("change", [
    {"gene_ptr": [0, 3, 2]},                                  # gene_ptr not monotone
    {"gene_ptr": [1, 2, 3]},                                  # gene_ptr[0] != 0
    {"gene_ptr": [0, 2, 4]},                                  # gene_ptr[-1] beyond the entries
    {"cell": [0, 3, 1]},                                      # cell out of range
    {"cell": [0, -1, 1]},                                     # negative cell
    {"cell": [2, 0, 1]},                                      # cells of a gene not increasing
    {"cell": [1, 1, 1]},                                      # a cell twice in a gene
    {"val": [1.0, -2.0, 3.0]},                                # a negative value
    {"val": [1.0, np.nan, 3.0]},                              # NaN
    {"val": [1.0, np.inf, 3.0]},                              # infinite
    {"sf": [1.0, 1.0, -1.0]},                                 # a negative scaled value
    {"val": [1.0, 3e38, 3.0], "sf": [1.0, 1.0, 10.0]},       # the float32 product overflows
    {"set_ptr": [0, 0, 3]},                                   # empty test set
    {"set_ptr": [0, 3, 2]},                                   # set_ptr not monotone
    {"set_ptr": [1, 2, 3]},                                   # set_ptr[0] != 0
    {"members": [0, 1, 3]},                                   # member out of range
    {"members": [0, -1, 2]},                                  # negative member
    {"pair_test": [0, 2], "pair_ctrl": [1, 1]},               # a pair names a set that does not exist
    {"pair_test": [1], "pair_ctrl": [0], "set_ptr": [0, 3, 3]},   # the pair's test set is empty
    {"pair_test": [0]},                                       # pair_ctrl missing
    {"exp_frac_thresh": np.nan},
    {"matrix2": ([0, 1], [0], [1.0], [1.0])},                 # the second matrix holds another number of genes
    {"matrix2": ([0, 1, 1], [0], [1.0], [1.0, 1.0]), "pair_test": [0, 1], "pair_ctrl": [1, 0]},   # test and control, two matrices
    {"matrix2": ([0, 1, 1], [0], [1.0], [1.0, 1.0])},         # control member 2 is no cell of the second matrix
])
def test_bad_arguments_are_refused_before_any_device(change):
    with pytest.raises(ValueError):
        nabo_amd.de_test_csc(**dict(GOOD, **change))


def test_null_outputs_are_refused():
    L = _lib.lib()
    a = {k: np.ascontiguousarray(v, dtype=t) for (k, v), t in zip(GOOD.items(), (np.int64, np.int32, np.float32, np.float32, np.int64, np.int64))}
    st = L.nabo_de_test(0, 2, 3, a["gene_ptr"].ctypes.data, a["cell"].ctypes.data, a["val"].ctypes.data, a["sf"].ctypes.data, 0, None, None,
                        None, None, 2, a["set_ptr"].ctypes.data, a["members"].ctypes.data, 0, None, None, 0.25, 1.0, 0, *[None] * 10)
    assert st == _lib.E_INVALID and b"output" in L.nabo_last_error()
    assert L.nabo_de_last_device_ms(None, None) == _lib.E_INVALID


def test_no_device_is_a_loud_failure():
    if nabo_amd.device_count() > 0:
        pytest.skip("a GPU is visible here; the no-device path is covered on the CPU box")
    with pytest.raises(nabo_amd.NaboError) as e:
        nabo_amd.de_test_csc(**GOOD)
    assert "no HIP device" in str(e.value)


def test_restatement_reproduces_reference_tables(golden):
    """the restatement as the device step: row sets, exp_frac and rbc exactly, the rest within the tolerances; the
    statuses cover both p methods, empty groups and both kinds of skip"""
    d = golden("de")
    seen = set()

    def step(*a):
        r = dref.de_step(*a)
        seen.update(np.unique(r["status"]).tolist())
        assert (r["u2"] >= 0).all() and (r["tie"] >= 0).all() and (r["u2"] <= 2 * r["n1"] * r["n2"]).all()
        return r
    assert dref.check_cases(d, step, *tolerances(d)) >= 600
    assert seen == {dref.SKIP_GENE, dref.SKIP_PAIR, dref.ASYMPTOTIC, dref.EXACT, dref.EMPTY}


def test_find_cluster_markers_host_logic_reproduces_reference(golden):
    d = golden("de")
    assert dref.check_markers(d, dref.de_step, *tolerances(d)) >= 200


def test_generator_margins_hold(golden):
    """no golden pair's log2_fc is within the tolerance of its threshold, so the skip decisions must match exactly"""
    d = golden("de")
    tol, _ = tolerances(d)
    assert 0 < tol < 1e-5
    for case in dref.golden_cases(d):
        if case["result"] != "ok":
            continue
        genes, m1, m2, test_idx, groups = dref.case_inputs(d, case)
        sp, mem = _de._flatten([test_idx] + groups)
        n = len(groups)
        r = dref.de_step(len(genes), m1, m2, sp, mem, np.zeros(n, np.int32), np.arange(1, n + 1, dtype=np.int32),
                         case["exp_frac_thresh"], case["log2_fc_thresh"])
        lfc = r["log2_fc"][(r["status"] != dref.SKIP_GENE) & (r["status"] != dref.EMPTY)]
        lfc = lfc[np.isfinite(lfc)]
        assert lfc.size == 0 or np.abs(lfc - case["log2_fc_thresh"]).min() > tol, case["name"]


def test_carry_over_of_an_empty_group():
    """rows of an empty group take rbc and pval from the last tested group of the same gene, 0 and 1 if none"""
    st = np.array([[4, 2, 4, 1, 3, 4], [4, 4, 1, 0, 0, 4], [0, 0, 0, 0, 0, 0]], dtype=np.int32)
    res = {"status": st, "rbc": np.arange(18, dtype=np.float64).reshape(3, 6) / 10, "pval": np.arange(18, dtype=np.float64).reshape(3, 6) / 100,
           "log2_fc": np.where(st == 4, np.nan, 1.5), "nonzero_test": np.full((3, 6), 3), "n1": np.full((3, 6), 4)}
    g, i, ef, rbc, lfc, p = _de._rows_from_pairs(res, np.arange(6))
    assert g.tolist() == [0, 0, 0, 0, 0, 1, 1, 1] and i.tolist() == [0, 1, 2, 4, 5, 0, 1, 5]
    assert rbc.tolist() == [0.0, 0.1, 0.1, 0.4, 0.4, 0.0, 0.0, 0.0] and p.tolist() == [1.0, 0.01, 0.01, 0.04, 0.04, 1.0, 1.0, 1.0]
    assert (ef == 0.75).all() and np.isnan(lfc[[0, 2, 4, 5, 6, 7]]).all()


def test_fdr_bh_ties_and_order():
    p = np.array([0.04, 0.01, 0.04, 0.5, 0.01, 1.0, 0.04])
    q = _de._fdr_bh(p)
    assert q[0] == q[2] == q[6] and q[1] == q[4] and (q <= 1).all() and q[5] == 1.0
    assert np.array_equal(q, [0.04 / (5 / 7), 0.01 / (2 / 7), 0.04 / (5 / 7), 0.5 / (6 / 7), 0.01 / (2 / 7), 1.0, 0.04 / (5 / 7)])
    # a single row has no q-value and the filter drops it; equal q-values keep the emission order
    rows = (np.array([0]), np.array([0]), np.array([0.5]), np.array([0.1]), np.array([2.0]), np.array([0.001]))
    assert _de._table_from_rows(["a"], rows, "T", ["x"], 2)["gene"] == []
    rows = (np.array([0, 1, 2]), np.array([0, 0, 0]), np.full(3, 0.5), np.zeros(3), np.ones(3), np.array([0.02, 0.001, 0.02]))
    t = _de._table_from_rows(["a", "b", "c"], rows, "T", ["x"], 2)
    assert t["gene"] == ["b", "a", "c"] and t["test_group"] == ["T"] * 3 and t["log2_fc"].dtype == np.float32
    assert _de._table_from_rows(["a", "b", "c"], rows, "T", ["x"], 0.01)["gene"] == ["b"]


def test_exact_p_of_the_restatement():
    """the U distribution by its generating function against a brute-force enumeration"""
    from itertools import combinations
    for m, n in ((1, 1), (2, 3), (3, 5), (4, 4), (2, 9)):
        counts = {}
        for pos in combinations(range(m + n), m):
            u = sum(p - k for k, p in enumerate(pos))
            counts[u] = counts.get(u, 0) + 1
        total = sum(counts.values())
        for u in range(m * n + 1):
            want = min(1.0, 2.0 * sum(c for k, c in counts.items() if k >= max(u, m * n - u)) / total)
            assert abs(dref.exact_p(m, n, 2 * u) - want) < 1e-15, (m, n, u)
            assert abs(dref.exact_p(n, m, 2 * u) - want) < 1e-15


# ---- the edge cases: restatement against the dense reference ----------------------------------------------------------
def references(name, _cache={}):
    """(dense reference, restatement's arrays) of an edge case, computed once"""
    if name not in _cache:
        a = edges.args(edges.case(name))
        _cache[name] = (dense.dense_step(*a), dref.de_step(*a))
    return _cache[name]


def margins_hold(case, want, tol):
    """every finite reference log2_fc is farther from the threshold than the tolerance, so a skip cannot flip"""
    lfc = [w["log2_fc"] for row in want for w in row if w["status"] not in (dref.SKIP_GENE, dref.EMPTY)]
    lfc = [x for x in lfc if math.isfinite(x)]
    if case.get("exact_threshold"):
        return bool(lfc) and all(x == case["log2_fc_thresh"] for x in lfc)
    return all(abs(x - case["log2_fc_thresh"]) > tol for x in lfc)


@pytest.mark.parametrize("name", edges.all_names())
def test_dense_reference_and_restatement_agree_on_the_edge_cases(golden, name):
    """two statements of the step written differently: integers and statuses exactly, z within its float64 bound, p and
    log2_fc within theirs; and the margin that keeps the device's skip decisions unambiguous"""
    tol, p_rel = tolerances(golden("de"))
    want, step = references(name)
    worst = dense.check_against_dense(step, want, tol, p_rel, name)
    print("%s: largest z error %.3f of its bound" % (name, worst))
    assert margins_hold(edges.case(name), want, tol), name


def test_edge_cases_reach_their_edges():
    """what each family is there for is really in its cases"""
    def get(name, k):
        return [[w.get(k) for w in row] for row in references(name)[0]]

    def st(name):
        return np.array(get(name, "status"))
    assert (st("exact_sweep_to_8") == dref.EXACT).all() and (st("exact_large_n1") == dref.EXACT).all()
    assert 1.0 in get("exact_sweep_to_8", "rbc")[0] and -1.0 in get("exact_sweep_to_8", "rbc")[1]          # U at both ends
    z = get("runs_all_equal", "z")
    assert z[0][0] is None and z[1][0] is not None                    # the zero-variance pair
    assert sorted(np.unique(st("zeros_counted")).tolist()) == [dref.SKIP_GENE, dref.ASYMPTOTIC]
    assert st("zeros_counted")[16, 0] == dref.ASYMPTOTIC and get("zeros_counted", "nonzero_test")[16][0] == 3
    assert (st("thresh_frac_on_threshold")[:, 0] == [dref.ASYMPTOTIC, dref.SKIP_GENE, dref.SKIP_GENE, dref.SKIP_GENE, dref.ASYMPTOTIC]).all()
    assert (st("thresh_all_zero_test_skipped")[2:4, 0] == [dref.SKIP_PAIR, dref.ASYMPTOTIC]).all()
    assert (st("thresh_frac_above_one") == dref.SKIP_GENE).all()
    assert (st("thresh_log2_fc_on_threshold") >= dref.ASYMPTOTIC).all()
    assert dref.EMPTY in st("sets_memberships") and dref.EMPTY in st("two_matrices")
    t0 = 2 * ((1 << 20) - 8)
    tie = get("limit_just_below", "tie")[0]
    assert 2 ** 63 - 2 ** 48 < t0 ** 3 < 2 ** 63 and all(t0 ** 3 - t0 <= t < 2 ** 63 for t in tie)
    for k in (1, 2, 8, 9, 16, 17):
        assert any(n.startswith("chunks_nseg_%d_" % k) for n in edges.FAMILIES["chunks"])


# ---- the exact p of the library, compiled for the host ----------------------------------------------------------------
@pytest.fixture(scope="module")
def exact_lib():
    shim = os.path.join(REPO, "tests", "host_shim")
    so = os.path.join(shim, "build", "libnabo_de_exact_host.so")
    deps = [os.path.join(shim, "de_exact_host.cpp"), os.path.join(REPO, "nabo_amd", "csrc", "de_exact.h"), os.path.join(REPO, "include", "nabo_knn.h")]
    os.makedirs(os.path.dirname(so), exist_ok=True)
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-fPIC", "-shared", deps[0], "-o", so])
    L = C.CDLL(so)
    L.nabo_last_error.restype = C.c_char_p
    L.nabo_host_de_exact_pvalue.argtypes = [C.c_int64, C.c_int64, C.c_int64, C.POINTER(C.c_double)]

    def p_of(n1, n2, u2):
        p = C.c_double(-1.0)
        rc = L.nabo_host_de_exact_pvalue(n1, n2, u2, C.byref(p))
        return rc, p.value, L.nabo_last_error().decode()
    return p_of


def test_exact_p_small_samples_every_u(exact_lib):
    """every (n1, n2) up to 8 x 8, both orders, every U: Python integers within 4 * 2^-53 (two conversions, one division)"""
    for n1 in range(1, 9):
        for n2 in range(1, 9):
            for u in range(n1 * n2 + 1):
                rc, p, _ = exact_lib(n1, n2, 2 * u)
                want = dref.exact_p(n1, n2, 2 * u)
                assert rc == 0 and abs(p - want) <= dense.P_EXACT_REL * want, (n1, n2, u, p, want)
    assert exact_lib(8, 8, 64)[1] == 1.0 and exact_lib(3, 2, 0)[1] == 2.0 / 10


@pytest.mark.parametrize("n1,n2", [(9, 8), (1000, 8), (174439, 8), (174440, 8), (226220, 8), (300000, 7), (8, 226220), (1 << 21, 1)])
def test_exact_p_large_samples(exact_lib, n1, n2):
    """up to the last binomial below 2^127 (C(226228, 8) has 127 bits), at both ends of U and where the 128-bit ring has
    wrapped on the way (K = 20000 coefficients)"""
    mn = n1 * n2
    assert math.comb(n1 + n2, n2) < 2 ** 127
    for u in (mn, mn - 1, mn - 17, 3, 0, mn - min(mn // 2, 20000)):
        rc, p, msg = exact_lib(n1, n2, 2 * u)
        want = dref.exact_p(n1, n2, 2 * u)
        assert rc == 0 and abs(p - want) <= dense.P_EXACT_REL * want, (n1, n2, u, p, want, msg)


def test_exact_p_limit_is_the_header_s(exact_lib):
    """include/nabo_de.h: NABO_E_UNSUPPORTED when C(n1 + n2, n1) >= 2^127, not before"""
    hdr = open(os.path.join(REPO, "include", "nabo_de.h")).read()
    assert "NABO_E_UNSUPPORTED when C(n1 + n2, n1) >= 2^127" in hdr
    assert math.comb(226220 + 8, 8) < 2 ** 127 <= math.comb(226221 + 8, 8)
    for n1, n2 in ((226221, 8), (8, 226221), (400000, 8), ((1 << 21) - 9, 8), (3000000, 7)):
        assert math.comb(n1 + n2, n2) >= 2 ** 127
        rc, p, msg = exact_lib(n1, n2, 2 * n1 * n2 - 6)
        assert rc == _lib.E_UNSUPPORTED and "%d and %d" % (n1, n2) in msg and p == -1.0, (n1, n2, rc, msg)
    rc, p, _ = exact_lib(226220, 8, 2 * 226220 * 8 - 6)                   # the next call works
    assert rc == 0 and abs(p - dref.exact_p(226220, 8, 2 * 226220 * 8 - 6)) <= dense.P_EXACT_REL * p
    # the largest 7-sample binomial below the limit and the first beyond it, by bisection
    lo, hi = 300000, 1 << 21
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if math.comb(mid + 7, 7) < 2 ** 127 else (lo, mid)
    assert math.comb(lo + 7, 7) < 2 ** 127 <= math.comb(hi + 7, 7)
    assert exact_lib(lo, 7, 2 * lo * 7)[0] == 0 and exact_lib(hi, 7, 2 * hi * 7)[0] == _lib.E_UNSUPPORTED
