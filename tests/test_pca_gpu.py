"""The PCA projection and the gene statistics on the MI355X (nabo_pca_project, nabo_gene_stats, nabo_amd._pca): through
the C ABI bit-equal to the tests' plain restatement and within the measured deviation of the reference's vectors
(tests/golden/pca.npz), in one chunk and in forced chunks; the edges; float32 products that underflow; a 300k-cell case
in a process of its own; the file-level functions with `Mapping` on what they write; and the plain-C consumer.

Bounds of the statistics against the restatement (exactly rounded sums): any summation order of n non-negative terms is
within (n - 1) 2^-53 of the exact sum, relatively, so m and nzm get n 2^-53; the variance's terms are non-negative too and
the sum of squared deviations is stationary in the mean, so the mean's own error enters at second order only, and the
factor 4 in 4 n 2^-53 covers the roundings of each term."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _pca_ref as pref
from test_mapping import _interpreter
from test_pca_cpu import build_pca_check

HERE = os.path.dirname(os.path.abspath(__file__))
EPS = 2.0 ** -53


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _check_stats(got, want, n, what):
    assert np.array_equal(got["ncells"], want["ncells"]) and np.array_equal(got["valid"], want["valid"]), what
    for k, bound in (("m", n * EPS), ("nzm", n * EPS), ("variance", 4 * n * EPS)):
        rel = np.abs(got[k] - want[k]) / np.where(want[k] != 0, np.abs(want[k]), 1.0)
        print("%s: %s relative difference %.3g (allowed %.3g)" % (what, k, rel.max() if rel.size else 0.0, bound))
        assert (rel <= bound).all(), (what, k)
        assert (got[k][want["valid"] == 0] == 0).all(), (what, k)


@pytest.mark.gpu
@pytest.mark.parametrize("budget", [0, 8192])
def test_golden_projections_bit_equal_to_the_restatement(gpu_lib, golden, budget):
    """every golden projection through the C ABI; with an 8 kB budget the rows go in several chunks"""
    from nabo_amd import _pca
    d = golden("pca")
    tol = 4 * float(d["proj_dev"])
    for name, _, kw, Zref in pref.projection_calls(d):
        Z = gpu_lib.pca_project_csr(mem_budget=budget, **kw)
        ms, chunks = _pca.last_device_ms()
        print("%s, budget %d: %d chunks, device ms %s" % (name, budget, chunks, ms))
        assert chunks > 4 if budget else chunks == 1, (name, chunks)
        want = pref.project(**kw)
        assert _same(Z, want), (name, np.argwhere(_bits(Z) != _bits(want))[:5].tolist())
        dev = pref.row_dev(Zref, Z)
        print("%s: deviation from the reference's vectors %.3g (allowed %.3g)" % (name, dev, tol))
        assert dev <= tol, name
    # a budget one row does not fit in is refused, not exceeded
    with pytest.raises(gpu_lib.NaboError) as e:
        gpu_lib.pca_project_csr(mem_budget=64, **kw)
    assert "budget" in str(e.value)


@pytest.mark.gpu
def test_golden_statistics(gpu_lib, golden):
    d = golden("pca")
    keep_cells, keep_genes = d["r_keep_cells"], pref.keep_mask(d, "r")
    got = gpu_lib.gene_stats_csc(*pref.csc_of(d, "r"), keep_cells=keep_cells, keep_genes=keep_genes)
    want = pref.gene_stats(*pref.csc_of(d, "r"), keep_cells=keep_cells, keep_genes=keep_genes)
    _check_stats(got, want, len(keep_cells), "golden")
    assert got["ncells"].dtype == np.int64 and got["valid"].dtype == np.uint8 and got["m"].dtype == np.float64
    ref = pref.golden_stats(d)
    assert np.array_equal(got["ncells"], ref["ncells"]) and np.array_equal(got["valid"], ref["valid"])
    for k, dev, stored in zip(("m", "nzm", "variance"), pref.stats_devs(ref, got), (d["m_dev"], d["nzm_dev"], d["var_dev"])):
        print("%s: deviation from the reference %.3g (allowed %.3g)" % (k, dev, 4 * float(stored)))
        assert dev <= 4 * float(stored), k
    # without the lists: all cells, all genes
    got = gpu_lib.gene_stats_csc(*pref.csc_of(d, "t"))
    _check_stats(got, pref.gene_stats(*pref.csc_of(d, "t")), len(d["t_cells"]), "target, nothing dropped")


def edge_matrix(n_raw, G, C, seed):
    """12 cells: cell 0 empty, cell 1 with unselected genes only, cell 2 with every raw gene (several loads of 64 entries
    when n_raw > 64), the others random; stored zeros among the values"""
    rng = np.random.default_rng(seed)
    sel = np.sort(rng.permutation(n_raw)[:min(G, n_raw)])
    gene_pos = np.full(n_raw, -1, dtype=np.int32)
    gene_pos[sel] = rng.permutation(G)[:sel.shape[0]]
    unsel = np.nonzero(gene_pos < 0)[0]
    rows = [np.zeros(0, np.int64), unsel[:max(1, unsel.shape[0] // 2)], np.arange(n_raw)]
    rows += [np.sort(rng.permutation(n_raw)[:rng.integers(1, n_raw + 1)]) for _ in range(9)]
    cell_ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    gene = np.concatenate(rows).astype(np.int32)
    val = rng.poisson(1.0, gene.shape[0]).astype(np.float32) * np.float32(0.75)
    val[cell_ptr[2]:cell_ptr[3]] += np.float32(0.75)            # cell 2: every gene positive
    sf = (0.5 + rng.random(len(rows))).astype(np.float32)
    return dict(cell_ptr=cell_ptr, gene=gene, val=val, sf=sf, gene_pos=gene_pos, mu=rng.random(G), sigma=0.5 + rng.random(G),
                mean=rng.normal(size=G), components=rng.normal(size=(C, G)))


@pytest.mark.gpu
@pytest.mark.parametrize("n_raw,G,C", [(200, 60, 1), (200, 60, 50), (200, 60, 64), (200, 60, 65), (200, 60, 200), (300, 150, 257), (40, 1, 8),
                                       (40, 1, 1), (30, 45, 7)])
def test_projection_edges(gpu_lib, n_raw, G, C):
    """an empty cell (the bias), a cell with unselected genes only (the bias too), rows repeated and in reverse order,
    G = 1, component counts around the wave width, selected genes no raw gene maps to"""
    kw = edge_matrix(n_raw, G, C, seed=n_raw + G + C)
    Z = gpu_lib.pca_project_csr(**kw)
    want = pref.project(**kw)
    assert Z.shape == (12, C) and _same(Z, want), np.argwhere(_bits(Z) != _bits(want))[:5].tolist()
    bias = pref.bias_of(kw["mu"], kw["sigma"], kw["mean"], kw["components"])
    assert _same(Z[0], bias) and _same(Z[1], bias) and not _same(Z[2], bias)
    rows = np.array([11, 10, 9, 8, 7, 6, 5, 4, 3, 2, 1, 0, 2, 2, 0, 11])
    assert _same(gpu_lib.pca_project_csr(rows=rows, **kw), want[rows])
    assert _same(gpu_lib.pca_project_csr(rows=rows, mem_budget=20000 + 16 * C, **kw), want[rows])
    assert gpu_lib.pca_project_csr(rows=np.zeros(0, np.int64), **kw).shape == (0, C)


@pytest.mark.gpu
def test_statistics_edges(gpu_lib):
    """a gene with every cell listed, an empty column, a column of stored zeros only, a gene the mask drops, a keep list
    of a single cell"""
    rng = np.random.default_rng(5)
    n_cells = 500
    cols = [np.arange(n_cells), np.zeros(0, np.int64), np.arange(0, n_cells, 7), np.arange(3, n_cells, 2)]
    cols += [np.sort(rng.permutation(n_cells)[:rng.integers(1, n_cells)]) for _ in range(20)]
    gene_ptr = np.concatenate([[0], np.cumsum([len(c) for c in cols])]).astype(np.int64)
    cell = np.concatenate(cols).astype(np.int32)
    val = (rng.poisson(2.0, cell.shape[0])).astype(np.float32)
    val[gene_ptr[0]:gene_ptr[1]] += 1                            # gene 0: positive in every cell
    val[gene_ptr[2]:gene_ptr[3]] = 0                             # gene 2: listed, never positive
    sf = (0.5 + rng.random(n_cells)).astype(np.float32)
    m = (gene_ptr, cell, val, sf)
    mask = np.ones(len(cols), np.uint8)
    mask[3] = 0
    for keep_cells in (None, np.array([17]), np.array([499, 0, 250]), rng.permutation(n_cells)[:333]):
        got = gpu_lib.gene_stats_csc(*m, keep_cells=keep_cells, keep_genes=mask)
        want = pref.gene_stats(*m, keep_cells=keep_cells, keep_genes=mask)
        n = n_cells if keep_cells is None else len(keep_cells)
        _check_stats(got, want, n, "keep %s" % (None if keep_cells is None else len(keep_cells)))
        assert got["valid"][0] == 1 and got["ncells"][0] == n and not got["valid"][1] and not got["valid"][2] and not got["valid"][3]
        assert got["m"][0] == got["nzm"][0]
        if n == 1:
            assert (got["variance"] == 0).all()


@pytest.mark.gpu
def test_float32_products_that_underflow(gpu_lib):
    """"one float32 product" where it leaves the normal range: values of 1e-30f in cells with sf = 1e-10f (cells 3 and 11:
    the product is a positive subnormal) and with sf = 1e-20f (cells 7 and 13: the product is exactly 0), among ordinary
    cells.  pca_project_csr is the restatement bit for bit, also with mu = mean = 0, where the bias is 0 and the
    subnormal products are all a row holds; gene_stats_csc counts the subnormal product as positive and the underflowed
    one not: gene 0 (cells 3 and 11 only) is valid with ncells 2, gene 1 (cells 7 and 13 only) is not valid, gene 2 is
    listed by all four and by ordinary cells"""
    rng = np.random.default_rng(31)
    n_cells, n_raw, G, C = 40, 50, 30, 5
    tiny_cells, zero_cells = [3, 11], [7, 13]
    X = np.where(rng.random((n_cells, n_raw)) < 0.4, 0.75 + 0.75 * rng.poisson(1.0, (n_cells, n_raw)), 0).astype(np.float32)
    X[:, :2] = 0
    X[tiny_cells + zero_cells, 2] = 1
    X[tiny_cells, 0] = 1
    X[zero_cells, 1] = 1
    X[rng.random((n_cells, n_raw)) < 0.05] = np.float32(1e-30)         # and a few among the ordinary cells' values
    X[tiny_cells + zero_cells] = np.where(X[tiny_cells + zero_cells] > 0, np.float32(1e-30), 0)
    X[:, 0] = np.where(np.isin(np.arange(n_cells), tiny_cells), X[:, 0], 0)
    X[:, 1] = np.where(np.isin(np.arange(n_cells), zero_cells), X[:, 1], 0)
    sf = (0.5 + rng.random(n_cells)).astype(np.float32)
    sf[tiny_cells], sf[zero_cells] = np.float32(1e-10), np.float32(1e-20)
    P = X * sf[:, None]
    assert P.dtype == np.float32 and ((P[tiny_cells] > 0) == (X[tiny_cells] > 0)).all() and (P[tiny_cells] < np.finfo(np.float32).tiny).all()
    assert (X[zero_cells] > 0).sum() > 20 and not P[zero_cells].any() and (X[tiny_cells] > 0).sum() > 20
    ci, gi = np.nonzero(X)
    cell_ptr = np.concatenate([[0], np.cumsum(np.bincount(ci, minlength=n_cells))]).astype(np.int64)
    gene_pos = np.full(n_raw, -1, dtype=np.int32)
    gene_pos[np.sort(rng.permutation(n_raw - 3)[:G - 3] + 3)] = rng.permutation(G - 3) + 3
    gene_pos[:3] = [0, 1, 2]
    kw = dict(cell_ptr=cell_ptr, gene=gi.astype(np.int32), val=X[ci, gi], sf=sf, gene_pos=gene_pos, mu=rng.random(G), sigma=0.5 + rng.random(G),
              mean=rng.normal(size=G), components=rng.normal(size=(C, G)))
    Z, want = gpu_lib.pca_project_csr(**kw), pref.project(**kw)
    assert _same(Z, want), np.argwhere(_bits(Z) != _bits(want))[:5].tolist()
    kw0 = dict(kw, mu=np.zeros(G), mean=np.zeros(G))
    Z, want = gpu_lib.pca_project_csr(**kw0), pref.project(**kw0)
    assert (want[tiny_cells] != 0).all() and (np.abs(want[tiny_cells]) < 1e-36).all() and not want[zero_cells].any()
    assert _same(Z, want), np.argwhere(_bits(Z) != _bits(want))[:5].tolist()
    # the same entries by gene
    gj, cj = np.nonzero(X.T)
    m = (np.concatenate([[0], np.cumsum(np.bincount(gj, minlength=n_raw))]).astype(np.int64), cj.astype(np.int32), X[cj, gj], sf)
    for keep_cells in (None, np.array(tiny_cells + zero_cells + [0, 1, 2, 20])):
        got = gpu_lib.gene_stats_csc(*m, keep_cells=keep_cells)
        want = pref.gene_stats(*m, keep_cells=keep_cells)
        kept = np.arange(n_cells) if keep_cells is None else keep_cells
        assert want["ncells"][:2].tolist() == [2, 0] and want["valid"][:2].tolist() == [1, 0] and 0 < want["m"][0] < 1e-39
        assert want["ncells"][2] == 2 + (P[np.setdiff1d(kept, tiny_cells + zero_cells), 2] > 0).sum()
        _check_stats(got, want, len(kept), "underflow, keep %s" % (None if keep_cells is None else len(keep_cells)))


@pytest.mark.gpu
def test_sized_case_300k_cells(gpu_lib):
    """300 000 cells x 8 000 raw genes at about 4 % density, 1 500 selected genes, 50 components, under a time limit of
    its own; prints the device ms and asserts no speed"""
    r = subprocess.run([sys.executable, os.path.join(HERE, "_pca_sized_case.py")], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       universal_newlines=True, timeout=840)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][len("RESULT "):])
    print(json.dumps(res, indent=1))
    assert 0.035 < res["density"] < 0.045
    assert res["chunks_one"] == 1 and res["chunks_chunked"] > 4 and res["chunks_equal"]
    assert res["rows_equal"] and res["rows_call_equal"]
    assert res["stats_exact"] and res["valid_genes"] > 7000
    for k in ("m", "nzm", "variance"):
        assert res[k + "_rel"] <= res[k + "_bound"], k


@pytest.mark.gpu
def test_file_level_functions_and_mapping(gpu_lib):
    py = _interpreter()
    if py is None:
        pytest.skip("no interpreter with h5py in this image")
    r = subprocess.run([py, os.path.join(HERE, "_pca_case.py")], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       universal_newlines=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][len("RESULT "):])
    assert res["checked"] == 39 and res["differ"] == [], res


@pytest.mark.gpu
def test_plain_c_consumer_reproduces_a_golden_call(gpu_lib, golden, tmp_path):
    exe = build_pca_check(tmp_path)
    d = golden("pca")
    _, _, kw, _ = pref.projection_calls(d)[1]                    # the target sample: fill_missing genes, an empty cell
    G, C = kw["mu"].shape[0], kw["components"].shape[0]
    rows = kw["rows"][::-1][:50]
    text = "%d %d %d %d %d\n" % (len(kw["sf"]), len(kw["gene_pos"]), G, C, len(rows))
    text += " ".join(str(int(x)) for x in kw["cell_ptr"]) + "\n" + "\n".join("%d %r" % (int(g), float(v)) for g, v in zip(kw["gene"], kw["val"])) + "\n"
    text += " ".join(repr(float(x)) for x in kw["sf"]) + "\n" + " ".join(str(int(x)) for x in kw["gene_pos"]) + "\n"
    for k in ("mu", "sigma", "mean"):
        text += " ".join(repr(float(x)) for x in kw[k]) + "\n"
    text += " ".join(repr(float(x)) for x in kw["components"].ravel()) + "\n" + " ".join(str(int(x)) for x in rows) + "\n"
    r = subprocess.run([exe, "run"], input=text, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
    assert r.returncode == 0, r.stdout
    got = np.array([[float(x) for x in ln.split()[2:]] for ln in r.stdout.splitlines() if ln.startswith("row ")])
    want = pref.project(**dict(kw, rows=rows))
    assert _same(got, want)
