"""The exact PCA fit (include/nabo_pca_fit.h, nabo_amd/_pca.py) without a GPU: the header and its symbols, the refusals
before any device, the host logic -- eigen-decomposition, order, clipping, sign rule, the n_comps resets, missing genes --
with the device step replaced by numpy, against the tests' restatement (tests/_pca_fit_ref.py) on the golden sample
(tests/golden/pca_fit.npz, tools/gen_golden_pca_fit.py), and the GPU tests' bound on two legitimate summation orders."""
import os
import re
import subprocess

import numpy as np
import pytest

import nabo_amd
from nabo_amd import _lib, _pca

import _pca_fit_ref as fref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CACHE = {}


def numpy_cov_step(m, gene_pos, mu, sigma, rows):
    """a float64 numpy evaluation of the definition in the place of _pca._device_cov (pairwise sums, BLAS product)"""
    Y = fref.scaled_rows(m[1], m[2], m[3], m[4], gene_pos, mu, sigma, rows)
    mean = Y.sum(axis=0) / Y.shape[0]
    Yc = Y - mean
    return mean, (Yc.T @ Yc) / (Y.shape[0] - 1)


def restated(d, regime):
    if regime not in _CACHE:
        kw, sel = fref.fit_call(d, regime)
        Y = fref.scaled_rows(**kw)
        _CACHE[regime] = (kw, sel, Y) + fref.mean_cov(Y)
    return _CACHE[regime]


def test_header_is_plain_c99():
    for h in ("nabo_pca_fit.h", "nabo_pca.h"):
        r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-x", "c", "-I" + os.path.join(REPO, "include"),
                            os.path.join(REPO, "include", h)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
        assert r.returncode == 0, r.stdout


def test_library_exports_the_fit_symbols():
    src = open(os.path.join(REPO, "include", "nabo_pca_fit.h")).read()
    assert '#include "nabo_pca_fit.h"' in open(os.path.join(REPO, "include", "nabo_pca.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert sorted(set(re.findall(r"\b(nabo_[a-z0-9_]+)\s*\(", src))) == sorted(_lib.PCA_FIT_SYMBOLS)
    L = _lib.lib()
    for n in _lib.PCA_FIT_SYMBOLS:
        assert hasattr(L, n), n
    assert L.nabo_pca_cov_last_phase_ms(None) == _lib.E_INVALID


def test_public_names():
    for n in ("pca_cov_csr", "fit_pca_csr", "fit_pca", "FittedPCA"):
        assert n in nabo_amd.__all__ and callable(getattr(nabo_amd, n))


GOOD = dict(cell_ptr=[0, 2, 3, 3], gene=[0, 2, 1], val=[1.0, 2.0, 3.0], sf=[1.0, 1.0, 2.0], gene_pos=[0, 1, -1], mu=[0.5, 0.25], sigma=[1.0, 2.0])


@pytest.mark.parametrize("change", [
    {"rows": [1]},                                            # n_rows < 2
    {"rows": []},
    {"cell_ptr": [0, 3], "sf": [1.0]},                        # one cell, all cells
    {"sigma": [1.0, 0.0]},
    {"sigma": [np.inf, 1.0]},
    {"sigma": [1.0]},                                         # sigma of another length
    {"mu": [np.nan, 0.0]},
    {"gene_pos": [0, 0, -1]},                                 # a position twice
    {"gene_pos": [0, 2, -1]},                                 # a position >= G
    {"gene": [2, 0, 1]},                                      # genes of a cell not increasing
    {"val": [1.0, -2.0, 3.0]},
    {"rows": [0, 3]},                                         # a row that is no cell
    {"rows": [[0, 1]]},
])
def test_bad_arguments_are_refused_before_any_device(change):
    with pytest.raises(ValueError):
        nabo_amd.pca_cov_csr(**dict(GOOD, **change))
    with pytest.raises(ValueError):
        nabo_amd.fit_pca_csr(n_comps=1, **dict(GOOD, **change))


def test_null_outputs_and_no_device():
    L = _lib.lib()
    m = _pca._csr((GOOD["cell_ptr"], GOOD["gene"], GOOD["val"], GOOD["sf"]))
    t = _pca._fit_tables(GOOD["gene_pos"], GOOD["mu"], GOOD["sigma"])
    st = L.nabo_pca_cov(0, 3, 3, m[1].ctypes.data, m[2].ctypes.data, m[3].ctypes.data, m[4].ctypes.data, t[0].ctypes.data, 2, t[1].ctypes.data,
                        t[2].ctypes.data, 0, None, 0, None, None)
    assert st == _lib.E_INVALID and b"output" in L.nabo_last_error()
    if nabo_amd.device_count() == 0:
        with pytest.raises(nabo_amd.NaboError) as e:
            nabo_amd.pca_cov_csr(**GOOD)
        assert "no HIP device" in str(e.value)


def test_resident_bytes_restate_the_header():
    # 1 tile: 16 partial tiles; 136 tiles (2 000 genes): 8; 2 016 tiles (8 000 genes): 1
    assert _pca.cov_resident_bytes(1) == (131072 * 17 + 128 * 2048, 12 + 8 * 128)
    assert _pca.cov_resident_bytes(128) == _pca.cov_resident_bytes(1) and _pca.cov_resident_bytes(129)[1] == 12 + 8 * 256
    assert _pca.cov_resident_bytes(2000) == (136 * 131072 * 9 + 2048 * 2048, 12 + 8 * 2048)
    assert _pca.cov_resident_bytes(8000)[0] == 2016 * 131072 * 2 + 8064 * 2048


def test_fit_host_logic_against_the_restatement(golden):
    d = golden("pca_fit")
    raw = [str(x) for x in d["genes"]]
    m = _pca._csr((d["cell_ptr"], d["gene"], d["cval"], d["sf"]))
    for regime, n_comps in (("full", len(d["full_genes"])), ("trunc", 10)):
        kw, sel, Y, mean_w, cov_w = restated(d, regime)
        n, G = Y.shape
        want = fref.fit(mean_w, cov_w, n, n_comps)
        sp = {"genes": sel, "mu": d[regime + "_mu"], "sigma": d[regime + "_sigma"]}
        fit = _pca._fit_from_csr(raw, m, d["keep_cells"], sp, n_comps, step=lambda *a: (mean_w, cov_w))
        for k, v in want.items():
            assert np.array_equal(getattr(fit, k), v), (regime, k)
        assert fit.genes == sel and fit.n_samples_seen_ == n and fit.n_components_ == n_comps and fit.whiten is False
        # ordering, sign rule, orthonormal rows
        assert (np.diff(fit.explained_variance_) <= 0).all() and (fit.explained_variance_ >= 0).all()
        big = np.argmax(np.abs(fit.components_), axis=1)
        assert (fit.components_[np.arange(n_comps), big] > 0).all()
        assert np.abs(fit.components_ @ fit.components_.T - np.eye(n_comps)).max() < 1e-12
        assert np.allclose(fit.explained_variance_ratio_.sum(), 1.0 if regime == "full" else fit.explained_variance_.sum() / np.trace(cov_w))
        assert np.allclose(fit.transform(Y).var(axis=0, ddof=1)[:10], fit.explained_variance_[:10], rtol=1e-9)
        # with a numpy step: another summation order, the reference within 4 x the measured deviation in the exact regime
        fit = _pca._fit_from_csr(raw, m, d["keep_cells"], sp, n_comps, step=numpy_cov_step)
        if regime == "full":
            devs = fref.full_devs(d, fit.mean_, fit.explained_variance_, fit.transform(Y))
            print("numpy step against the reference: %s (allowed %.3g)" % (devs, 4 * float(d["fit_full_dev"])))
            assert max(devs) <= 4 * float(d["fit_full_dev"])
        else:
            assert fref.min_cosine(fit.components_, want["components_"]) > 1 - 1e-9
            assert fref.min_cosine(d["trunc_components"], want["components_"]) == pytest.approx(float(d["fit_trunc_cos"]), abs=1e-6)
    assert 0 < float(d["fit_full_dev"]) < 1e-9 and float(d["full_gap"]) > 1e-6 and float(d["fit_trunc_cos"]) < 0.9


def test_sign_rule_order_and_clipping():
    # eigenvalues 5, 2, 2, -1e-18: descending; the equal pair in eigh's order, reversed; the negative one reported as 0
    Q = np.linalg.qr(np.random.default_rng(2).normal(size=(4, 4)))[0]
    lam = np.array([2.0, 5.0, -1e-18, 2.0])
    cov = (Q * lam) @ Q.T
    cov = (cov + cov.T) / 2
    fit = nabo_amd.FittedPCA(np.zeros(4), cov, 11, 4)
    w, v = np.linalg.eigh(cov)
    assert np.allclose(fit.explained_variance_, [5, 2, 2, 0]) and fit.explained_variance_[3] == 0.0 and w[0] < 0
    for c in range(4):
        assert np.array_equal(np.abs(fit.components_[c]), np.abs(v[:, 3 - c]))
    assert np.allclose(fit.singular_values_, np.sqrt(np.array([5, 2, 2, 0]) * 10.0))
    assert np.array_equal(fit.var_, np.diag(cov)) and np.allclose(fit.explained_variance_ratio_, np.array([5, 2, 2, 0]) / np.trace(cov))
    # the entry of largest magnitude is positive, the first one on a tie
    s = np.sqrt(0.5)
    fit = nabo_amd.FittedPCA(np.zeros(2), np.array([[2.0, -1.0], [-1.0, 2.0]]), 5, 2)       # components (s, -s) and (s, s) up to sign
    assert np.allclose(fit.components_, [[s, -s], [s, s]]) and fit.components_[0, 0] > 0
    for bad in (dict(n=1), dict(n_comps=0), dict(n_comps=3), dict(cov=np.eye(3))):
        with pytest.raises(ValueError):
            nabo_amd.FittedPCA(**dict(dict(mean=np.zeros(2), cov=np.eye(2), n=5, n_comps=2), **bad))


def test_n_comps_resets_and_their_warnings(capsys):
    assert _pca._reset_n_comps(100, 250, 300) == 100 and capsys.readouterr().out == ""
    assert _pca._reset_n_comps(100, 40, 300) == 40
    assert capsys.readouterr().out.strip() == "WARNING: Number of components were reset to number of features i.e. 40"
    assert _pca._reset_n_comps(100, 250, 30) == 29
    assert capsys.readouterr().out.strip() == "WARNING: Number of components were reset to number of cells - 1 i.e. 29"
    assert _pca._reset_n_comps(100, 50, 30) == 29
    assert len(capsys.readouterr().out.strip().splitlines()) == 2
    assert _pca._reset_n_comps(30, 50, 30) == 30                  # the reference compares with >, not >=


def test_missing_genes_repeats_and_too_few_rows(golden, capsys):
    d = golden("pca_fit")
    raw = [str(x) for x in d["genes"]]
    m = _pca._csr((d["cell_ptr"], d["gene"], d["cval"], d["sf"]))
    sel = [str(x) for x in d["trunc_genes"]]
    sp = {"genes": sel + ["nobody"], "mu": np.append(d["trunc_mu"], 1.5), "sigma": np.append(d["trunc_sigma"], 0.5)}
    args = (raw, m, d["keep_cells"])
    with pytest.raises(KeyError) as e:
        _pca._fit_from_csr(*args, sp, 5, False, numpy_cov_step)
    assert "not found" in str(e.value)
    capsys.readouterr()
    fit = _pca._fit_from_csr(*args, sp, 5, True, numpy_cov_step)
    assert capsys.readouterr().out.strip() == "WARNING: 1 out %d genes are missing in this dataset" % (len(sel) + 1)
    assert fit.mean_[-1] == (0.0 - 1.5) / 0.5 and fit.var_[-1] == 0 and not fit.components_[:, -1].any()
    for bad_sp, rows, n_comps in ((dict(sp, genes=sel + sel[:1]), d["keep_cells"], 5), (None, d["keep_cells"], 5), (sp, d["keep_cells"][:1], 1),
                                  (sp, d["keep_cells"], 0), (sp, d["keep_cells"], len(sel) + 2)):
        with pytest.raises(ValueError):
            _pca._fit_from_csr(raw, m, rows, bad_sp, n_comps, True, numpy_cov_step)


def test_a_fitted_pca_goes_through_the_projection(golden):
    import _pca_ref as pref
    d = golden("pca_fit")
    kw, sel, Y, mean_w, cov_w = restated(d, "trunc")
    fit = nabo_amd.FittedPCA(mean_w, cov_w, Y.shape[0], 10, sel)
    sp = {"genes": sel, "mu": d["trunc_mu"], "sigma": d["trunc_sigma"]}
    m = _pca._csr((d["cell_ptr"], d["gene"], d["cval"], d["sf"]))

    def step(m, gene_pos, mu, sigma, mean, components, rows):
        return pref.project(m[1], m[2], m[3], m[4], gene_pos, mu, sigma, mean, components, rows)
    Z = _pca._project_from_csr([str(x) for x in d["genes"]], m, d["keep_cells"], fit, sp, False, step)
    assert Z.shape == (len(d["keep_cells"]), 10) and fref.row_dev(fit.transform(Y), Z) < 1e-12


def test_the_bound_holds_between_two_summation_orders():
    """two float64 numpy evaluations of the definition that sum in different orders -- rows as given through pairwise sums
    and BLAS, rows reversed through sequential cumulative sums -- stay within the GPU tests' bound of the restatement,
    and differ from it: the bound is not vacuous and a legitimate order does not violate it"""
    rng = np.random.default_rng(11)
    n, G = 400, 24
    Y = np.where(rng.random((n, G)) < 0.3, rng.gamma(2.0, 1.5, (n, G)), 0.0)
    Y = (np.float32(Y).astype(np.float64) - (4.0 + rng.random(G))) / (0.05 + 0.1 * rng.random(G))      # a mean far from 0
    mean_w, cov_w = fref.mean_cov(Y)
    e, B = fref.bounds(Y, mean_w)
    seen = 0
    for order in ("blas", "sequential"):
        if order == "blas":
            mean = Y.sum(axis=0) / n
            Yc = Y - mean
            cov = (Yc.T @ Yc) / (n - 1)
        else:
            mean = np.cumsum(Y[::-1], axis=0)[-1] / n
            Yc = Y[::-1] - mean
            cov = np.array([[np.cumsum(Yc[:, p] * Yc[:, q])[-1] for q in range(G)] for p in range(G)]) / (n - 1)
        dm, dc = np.abs(mean - mean_w), np.abs(cov - cov_w)
        print("%s: |d mean| / allowed %.3g, |d cov| / allowed %.3g" % (order, (dm / e).max(), (dc / B).max()))
        assert (dm <= e).all() and (dc <= B).all(), order
        seen += int(dm.any()) + int(dc.any())
    assert seen >= 2
    # and it is tight enough to catch a wrong value: one row left out of one column's sum
    bad = (Y.sum(axis=0) - np.where(np.arange(G) == 5, Y[7], 0.0)) / n
    assert not (np.abs(bad - mean_w) <= e).all()
    Yc = Y - mean_w
    assert not (np.abs((Yc[1:].T @ Yc[1:]) / (n - 1) - cov_w) <= B).all()


def test_integer_evaluation_of_the_exact_cases_equals_the_restatement():
    """fref.exact_mean_cov, which the GPU tests use where an fsum per entry takes too long, against fref.mean_cov bit for
    bit at 130 genes x 64 cells; and it refuses values that are not multiples of 1 / (4 n) or whose columns do not sum to 0"""
    from test_pca_fit_gpu import exact_case
    Y = fref.scaled_rows(**exact_case(130, 64))
    mean_w, cov_w = fref.mean_cov(Y)
    mean, cov = fref.exact_mean_cov(Y)
    assert np.array_equal(mean.view(np.int64), mean_w.view(np.int64)) and np.array_equal(cov.view(np.int64), cov_w.view(np.int64))
    assert np.count_nonzero(cov) > 0.95 * 128 * 128
    for bad in (Y + np.where(np.arange(64) == 9, 1.0 / 512, 0.0)[:, None], Y + 0.25):
        with pytest.raises(AssertionError):
            fref.exact_mean_cov(bad)
