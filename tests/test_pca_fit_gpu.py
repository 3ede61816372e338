"""The exact PCA fit on the MI355X (nabo_pca_cov, nabo_amd.pca_cov_csr / fit_pca_csr / fit_pca): bit-equal to the tests'
restatement (tests/_pca_fit_ref.py) where every operation is exact -- up to 2 049 genes, where the tile count sets the
number of splits --, within a derived bound of it elsewhere, within the measured deviation of the reference's exact
regime (tests/golden/pca_fit.npz), no worse than the reference's truncated fit, one sized case, the file-level function
with `Mapping` on what it leads to, and the refusals.

The bound against the restatement (exactly rounded sums), eps = 2^-53, n rows:  any order of n terms is within n eps of
the exact sum relative to the sum of the terms' magnitudes, so |d mean[p]| <= e_p = n eps A_p with A_p = sum|y| / n; for
the covariance Cauchy-Schwarz bounds the sum of |products| by s_p s_q (s_p the root of the column's centred sum of
squares), the mean's own error enters at second order only because the centred columns sum to zero (the n e_p e_q term,
and s'_p = s_p + sqrt(n) e_p), and the factor 4 covers the rounding of each centred value and product and whatever the
matrix pipe does inside a step:  |d cov[p][q]| <= (4 n eps s'_p s'_q + n e_p e_q) / (n - 1)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _pca_fit_ref as fref
from test_mapping import _interpreter

HERE = os.path.dirname(os.path.abspath(__file__))
_CACHE = {}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def exact_case(G, n):
    """integer counts <= 15, sf = 1, n a power of two, mu the exact column mean (a multiple of 1 / n), sigma a power of two:
    every y, product and partial sum is exact in float64 and the mean is exactly 0.  Cell 1 (cell 0 when n = 2) has no
    entry; with G >= 15 selected gene 3 is listed by no cell and selected gene 5 is a fill_missing gene"""
    rng = np.random.default_rng(1000 * G + n)
    n_raw = G + 6
    X = np.where(rng.random((n, n_raw)) < 0.3, rng.integers(1, 16, (n, n_raw)), 0).astype(np.float32)
    X[min(1, n - 2)] = 0
    X[n - 1, :] = np.maximum(X[n - 1, :], 1)                    # a cell that lists every raw gene
    raw_of = rng.permutation(n_raw)[:G]                          # selected gene p is raw gene raw_of[p]
    gene_pos = np.full(n_raw, -1, dtype=np.int32)
    gene_pos[raw_of] = np.arange(G)
    if G >= 15:
        X[:, raw_of[3]] = 0
        gene_pos[raw_of[5]] = -1
    ci, gi = np.nonzero(X)
    mu = np.zeros(G)
    for p in range(G):
        if gene_pos[raw_of[p]] == p:
            mu[p] = X[:, raw_of[p]].astype(np.float64).sum() / n     # integers below 2^14 over a power of two: exact
    sigma = 2.0 ** rng.integers(-2, 3, G)
    return dict(cell_ptr=np.concatenate([[0], np.cumsum(np.bincount(ci, minlength=n))]).astype(np.int64), gene=gi.astype(np.int32),
                val=X[ci, gi], sf=np.ones(n, np.float32), gene_pos=gene_pos, mu=mu, sigma=sigma)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [2, 64, 256, 1024])
@pytest.mark.parametrize("G", [1, 15, 16, 17, 130, 257])
def test_exact_arithmetic_cases_are_bit_equal(gpu_lib, G, n):
    """in one chunk and in forced chunks: a lane-map, tiling or chunk-boundary error shows as wrong bits whatever the order"""
    from nabo_amd import _pca
    kw = exact_case(G, n)
    Y = fref.scaled_rows(**kw)
    mean_w, cov_w = fref.mean_cov(Y)
    assert not mean_w.any() and (G < 15 or (not Y[:, 3].any() and not Y[:, 5].any() and not cov_w[3].any()))
    resident, row = _pca.cov_resident_bytes(G)
    per_row = row + 8 * int(np.diff(kw["cell_ptr"]).max())
    for rows_per_chunk in (None, max(1, n // 8)):
        budget = 0 if rows_per_chunk is None else resident + rows_per_chunk * per_row
        mean, cov = gpu_lib.pca_cov_csr(mem_budget=budget, **kw)
        chunks = _pca.last_device_ms()[1]
        assert chunks == 1 if rows_per_chunk is None else (chunks > 4 if n >= 64 else chunks == 2), (budget, chunks)
        assert _same(mean, mean_w), (budget, mean[:5])
        assert _same(cov, cov_w), (budget, np.argwhere(_bits(cov) != _bits(cov_w))[:5].tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("G,n,tiles,splits", [(1281, 256, 66, 16), (1409, 256, 78, 14), (2000, 256, 136, 8), (2049, 64, 153, 7)])
def test_exact_arithmetic_cases_at_the_workload_gene_counts(gpu_lib, G, n, tiles, splits):
    """the gene counts of a real selection, where the existing cases stop at 6 tiles: fit_tile_of's sqrt decode for tile
    numbers up to 152, cov_finish's gather for tile rows up to 16, and the partial tiles' layout [split][tile] with
    (1281, 256): 66 tiles, the last count with the constant 16 splits; (1409, 256): 78 tiles, 14 splits, the first where
    the tile count sets them; (2000, 256): 136 tiles and 8 splits, the workload's; (2049, 64): 153 tiles, 7 splits by the
    rule for the buffers but 4 launched over the 4 stages of 16 rows (one in the chunks of 8 rows).  In one chunk and in
    forced chunks, whose budget comes from _pca.cov_resident_bytes: its restated split rule is wrong if the chunk count
    is.  The mean is exactly 0, cov bit-equal to the integer evaluation and symmetric bit for bit."""
    from nabo_amd import _pca
    nt = -(-G // 128)
    assert nt * (nt + 1) // 2 == tiles and min(16, -(-1024 // tiles)) == splits
    kw = exact_case(G, n)
    Y = fref.scaled_rows(**kw)
    mean_w, cov_w = fref.exact_mean_cov(Y)
    assert not Y[:, 3].any() and not Y[:, 5].any() and not cov_w[3].any() and np.count_nonzero(cov_w) > 0.99 * (G - 2) ** 2
    resident, row = _pca.cov_resident_bytes(G)
    assert resident == tiles * 128 * 128 * 8 * (1 + splits) + nt * 128 * 8 * 256
    per_row = row + 8 * int(np.diff(kw["cell_ptr"]).max())
    for rows_per_chunk in (None, n // 8):
        budget = 0 if rows_per_chunk is None else resident + rows_per_chunk * per_row
        mean, cov = gpu_lib.pca_cov_csr(mem_budget=budget, **kw)
        chunks = _pca.last_device_ms()[1]
        assert chunks == 1 if rows_per_chunk is None else chunks > 4, (budget, chunks)
        assert _same(mean, mean_w), (budget, mean[:5])
        differ = np.argwhere(_bits(cov) != _bits(cov_w))
        assert _same(cov, cov_w), (budget, len(differ), differ[:5].tolist(), sorted(set(map(tuple, (differ // 128).tolist())))[:8])
        assert _same(cov, np.ascontiguousarray(cov.T)), "cov is not symmetric bit for bit"


@pytest.mark.gpu
def test_general_case_of_78_tiles_against_numpy(gpu_lib):
    """200 listed rows (permuted, repeated) x 1409 genes, the mean far from 0: 78 tiles and 14 splits with values that are
    not exact, against a float64 numpy evaluation with the bound of the module docstring (numpy's own sums are within it
    too), in one chunk and in three or more; two runs bit-equal, cov symmetric bit for bit"""
    from nabo_amd import _pca
    n, G = 200, 1409
    kw = general_case(n, G, listed=True, far=True, seed=n + G)
    Y = fref.scaled_rows(**kw)
    mean_w = Y.sum(axis=0) / n
    A = np.abs(Y).sum(axis=0) / n
    Yc = Y - mean_w
    cov_w = (Yc.T @ Yc) / (n - 1)
    e = n * fref.EPS * A
    s1 = np.sqrt((Yc * Yc).sum(axis=0)) + np.sqrt(n) * e
    B = (4 * n * fref.EPS * np.outer(s1, s1) + n * np.outer(e, e)) / (n - 1)
    assert (e > 0).all() and np.abs(mean_w).min() > 10
    resident, row = _pca.cov_resident_bytes(G)
    for budget in (0, resident + (n // 5) * (row + 8 * int(np.diff(kw["cell_ptr"]).max()))):
        mean, cov = gpu_lib.pca_cov_csr(mem_budget=budget, **kw)
        chunks = _pca.last_device_ms()[1]
        assert chunks == 1 if budget == 0 else chunks >= 3, chunks
        mean2, cov2 = gpu_lib.pca_cov_csr(mem_budget=budget, **kw)
        assert _same(mean, mean2) and _same(cov, cov2), "two runs of the same call differ"
        assert _same(cov, np.ascontiguousarray(cov.T)), "cov is not symmetric bit for bit"
        check_against(mean, cov, mean_w, cov_w, e, B, "n %d, G %d, budget %d" % (n, G, budget))


def general_case(n_cells, G, listed, far, seed):
    """float values and size factors, a sparse matrix over G + 40 raw genes; `listed`: n_cells rows drawn from 2 n_cells cells,
    permuted and with repeats; `far`: mu and sigma of another dataset, so that the mean is far from 0"""
    rng = np.random.default_rng(seed)
    n_all, n_raw = (2 * n_cells if listed else n_cells), G + 40
    X = np.where(rng.random((n_all, n_raw)) < 0.2, rng.gamma(2.0, 1.5, (n_all, n_raw)), 0).astype(np.float32)
    X[0] = 0
    ci, gi = np.nonzero(X)
    gene_pos = np.full(n_raw, -1, dtype=np.int32)
    gene_pos[rng.permutation(n_raw)[:G - 1]] = rng.permutation(G)[:G - 1]      # one selected gene is a fill_missing gene
    sf = (0.5 + rng.random(n_all)).astype(np.float32)
    mu, sigma = (5.0 + 3.0 * rng.random(G), 0.05 + 0.1 * rng.random(G)) if far else (0.6 * rng.random(G), 0.5 + rng.random(G))
    rows = rng.integers(0, n_all, n_cells) if listed else None
    if listed:
        rows[:2] = rows[2]                                           # a repeat for sure
    return dict(cell_ptr=np.concatenate([[0], np.cumsum(np.bincount(ci, minlength=n_all))]).astype(np.int64), gene=gi.astype(np.int32),
                val=X[ci, gi], sf=sf, gene_pos=gene_pos, mu=mu, sigma=sigma, rows=rows)


def check_against(mean, cov, mean_w, cov_w, e, B, what):
    dm, dc = np.abs(mean - mean_w), np.abs(cov - cov_w)
    print("%s: |d mean| / allowed at most %.3g (largest allowed %.3g), |d cov| / allowed at most %.3g (largest allowed %.3g)"
          % (what, (dm / e).max(), e.max(), (dc / B).max(), B.max()))
    assert (dm <= e).all(), what
    assert (dc <= B).all(), what


@pytest.mark.gpu
@pytest.mark.parametrize("n,G,listed,far", [(3, 37, False, False), (63, 37, True, True), (65, 150, False, True), (65, 150, True, False),
                                            (1000, 130, True, True), (1000, 40, False, False)])
def test_general_cases_against_the_restatement(gpu_lib, n, G, listed, far):
    from nabo_amd import _pca
    kw = general_case(n, G, listed, far, seed=n + G)
    Y = fref.scaled_rows(**kw)
    assert Y.shape == (n, G)
    mean_w, cov_w = fref.mean_cov(Y)
    e, B = fref.bounds(Y, mean_w)
    assert (e > 0).all() and (np.abs(mean_w).min() > 10 if far else True)
    resident, row = _pca.cov_resident_bytes(G)
    for budget in (0, resident + max(1, n // 5) * (row + 8 * int(np.diff(kw["cell_ptr"]).max()))):
        mean, cov = gpu_lib.pca_cov_csr(mem_budget=budget, **kw)
        chunks = _pca.last_device_ms()[1]
        assert chunks == 1 if budget == 0 else chunks >= 3, chunks
        mean2, cov2 = gpu_lib.pca_cov_csr(mem_budget=budget, **kw)
        assert _same(mean, mean2) and _same(cov, cov2), "two runs of the same call differ"
        assert _same(cov, np.ascontiguousarray(cov.T)), "cov is not symmetric bit for bit"
        check_against(mean, cov, mean_w, cov_w, e, B, "n %d, G %d, budget %d" % (n, G, budget))


def _golden_restated(d, regime):
    if regime not in _CACHE:
        kw, sel = fref.fit_call(d, regime)
        Y = fref.scaled_rows(**kw)
        _CACHE[regime] = (kw, sel, Y) + fref.mean_cov(Y)
    return _CACHE[regime]


@pytest.mark.gpu
def test_golden_full_regime_reproduces_the_reference(gpu_lib, golden):
    """n_comps = len(genes), where the reference's IncrementalPCA is exact: mean_, explained_variance_ and the projected kept
    cells within 4 x the deviation the generator measured between the reference and the restatement (the device sums in
    another order); the components only through the projected cells"""
    d = golden("pca_fit")
    kw, sel, Y, _, _ = _golden_restated(d, "full")
    tol = 4 * float(d["fit_full_dev"])
    fit = gpu_lib.fit_pca_csr(n_comps=len(sel), **kw)
    assert fit.components_.shape == (len(sel), len(sel)) and fit.n_samples_seen_ == len(d["keep_cells"]) and fit.whiten is False
    devs = fref.full_devs(d, fit.mean_, fit.explained_variance_, fit.transform(Y))
    print("deviation from the reference: mean %.3g, explained variance %.3g, projected cells %.3g (allowed %.3g)" % (devs + (tol,)))
    assert max(devs) <= tol


@pytest.mark.gpu
def test_golden_truncated_regime_is_no_worse_than_the_reference(gpu_lib, golden):
    d = golden("pca_fit")
    kw, sel, Y, _, cov_w = _golden_restated(d, "trunc")
    n, G = Y.shape
    fit = gpu_lib.fit_pca_csr(n_comps=10, **kw)
    V, Vref = fit.components_, d["trunc_components"]
    assert V.shape == Vref.shape == (10, G)
    assert np.abs(V @ V.T - np.eye(10)).max() <= 1e-12
    got, ref = float(np.trace(V @ cov_w @ V.T)), float(np.trace(Vref @ cov_w @ Vref.T))
    slack = G * n * fref.EPS * float(np.trace(cov_w))
    print("captured variance %.6f, the reference's %.6f of %.6f (slack %.3g); the reference's smallest cosine %.4f"
          % (got, ref, np.trace(cov_w), slack, float(d["fit_trunc_cos"])))
    assert got >= ref - slack
    # in order: each leading block captures no less than the reference's
    for c in range(1, 11):
        assert np.trace(V[:c] @ cov_w @ V[:c].T) >= np.trace(Vref[:c] @ cov_w @ Vref[:c].T) - slack, c
    assert (np.diff(fit.explained_variance_) <= 0).all()


@pytest.mark.gpu
def test_sized_case_20k_cells_600_genes(gpu_lib):
    """20 000 cells x 3 000 raw genes at 10 % density, 600 selected: 15 tiles, several partial tiles per tile; against a
    float64 numpy evaluation with the same bound (numpy's own sums are within it too)"""
    from nabo_amd import _pca
    rng = np.random.default_rng(7)
    n, n_raw, G = 20000, 3000, 600
    M = rng.random((n, n_raw), dtype=np.float32) < 0.1
    ci, gi = np.nonzero(M)
    del M
    val = (1 + rng.poisson(1.0, ci.shape[0])).astype(np.float32)
    sf = (0.5 + rng.random(n)).astype(np.float32)
    gene_pos = np.full(n_raw, -1, dtype=np.int32)
    gene_pos[rng.permutation(n_raw)[:G]] = rng.permutation(G)
    mu, sigma = 0.3 * rng.random(G), 0.5 + rng.random(G)
    cell_ptr = np.concatenate([[0], np.cumsum(np.bincount(ci, minlength=n))]).astype(np.int64)
    assert 0.09 < ci.shape[0] / (n * n_raw) < 0.11
    mean, cov = gpu_lib.pca_cov_csr(cell_ptr, gi.astype(np.int32), val, sf, gene_pos, mu, sigma)
    ms, chunks = _pca.last_device_ms()
    print("device ms %s, phases %s, %d chunk(s)" % (ms, _pca.last_cov_phase_ms(), chunks))
    Y = np.tile((0.0 - mu) / sigma, (n, 1))
    sel = gene_pos[gi] >= 0
    p = gene_pos[gi[sel]]
    Y[ci[sel], p] = ((val[sel] * sf[ci[sel]]).astype(np.float64) - mu[p]) / sigma[p]
    mean_w = Y.sum(axis=0) / n
    A = np.abs(Y).sum(axis=0) / n
    Y -= mean_w
    cov_w = (Y.T @ Y) / (n - 1)
    e = n * fref.EPS * A
    s1 = np.sqrt((Y * Y).sum(axis=0)) + np.sqrt(n) * e
    B = (4 * n * fref.EPS * np.outer(s1, s1) + n * np.outer(e, e)) / (n - 1)
    assert _same(cov, np.ascontiguousarray(cov.T))
    check_against(mean, cov, mean_w, cov_w, e, B, "20 000 x 600")


@pytest.mark.gpu
def test_file_level_fit_transform_and_mapping(gpu_lib):
    py = _interpreter()
    if py is None:
        pytest.skip("no interpreter with h5py in this image")
    r = subprocess.run([py, os.path.join(HERE, "_pca_fit_case.py")], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       universal_newlines=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][len("RESULT "):])
    assert res["checked"] == 11 and res["differ"] == [], res


@pytest.mark.gpu
def test_refusals(gpu_lib):
    from nabo_amd import _pca
    kw = general_case(20, 37, False, False, seed=3)
    resident, row = _pca.cov_resident_bytes(37)
    with pytest.raises(gpu_lib.NaboError) as e:
        gpu_lib.pca_cov_csr(mem_budget=resident + row - 1, **kw)
    assert "budget" in str(e.value)
    with pytest.raises(gpu_lib.NaboError) as e:
        gpu_lib.pca_cov_csr(mem_budget=4096, **kw)
    assert "budget" in str(e.value)
    with pytest.raises(ValueError):
        gpu_lib.pca_cov_csr(**dict(kw, rows=[4]))
    with pytest.raises(ValueError):
        gpu_lib.pca_cov_csr(**dict(kw, sigma=np.where(np.arange(37) == 9, 0.0, kw["sigma"])))
    pos = kw["gene_pos"].copy()
    pos[np.nonzero(pos < 0)[0][0]] = pos[np.nonzero(pos >= 0)[0][0]]
    with pytest.raises(ValueError):
        gpu_lib.pca_cov_csr(**dict(kw, gene_pos=pos))
