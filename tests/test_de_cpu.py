"""The Mann-Whitney DE test and cluster markers (include/nabo_de.h, nabo_amd/_de.py) without a GPU: the C header and its
symbols, argument checks, the no-device failure, the tests' plain restatement against the reference's tables
(tests/golden/de.npz, tools/gen_golden_de.py), and the host logic -- carry-over of an empty group, Benjamini-Hochberg,
ordering, filtering, marker counting -- with the device step replaced by that restatement."""
import os
import re
import subprocess

import numpy as np
import pytest

import nabo_amd
from nabo_amd import _de, _lib

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
