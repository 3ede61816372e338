#!/opt/conda/bin/python3.9
"""Golden vectors for the PCA fit of the reference (nabo/_dataset.py, fit_ipca :917-983 over get_scaled_values :846-915).

TEST INFRASTRUCTURE ONLY, run where the reference is mounted, with an interpreter that has h5py, pandas and sklearn:

    /opt/conda/bin/python3.9 tools/gen_golden_pca_fit.py

As tools/gen_golden_pca.py (whose loader and file writer it uses) it loads the reference's nabo/_dataset.py BY FILE PATH,
writes a seeded synthetic dataset as a Nabo-format HDF5 file into a temporary directory, runs the reference's own
functions on it and stores only DATA in tests/golden/pca_fit.npz.  The sample: 300 cells x 120 genes of counts with a
planted rank-6 structure (so that the leading eigenvalues are separated), a keep_cells_idx that drops cells, a
keep_genes_idx that drops genes, one kept gene without a nonzero value.  fit_ipca runs in two regimes:

  full   n_comps = len(genes) = 24, five batches.  IncrementalPCA is exact here; the script asserts it (deviation below
         1e-9) and that neighbouring eigenvalues are more than 1e-6 apart, relatively -- in fact it draws the genes until
         they are 2e-3 apart, so that the projected cells of two exact fits agree to rounding and not to rounding / gap.
  trunc  10 components of 40 genes, three batches: the reference's usual, approximate regime.

Stored per regime: the genes, mu and sigma, mean_, components_, explained_variance_, the projected kept cells; and
  fit_full_dev   the largest deviation of the reference's full fit from the tests' restatement (tests/_pca_fit_ref.py):
                 of mean_, of explained_variance_ relative to the largest, of the projected kept cells (row_dev);
  fit_trunc_cos  the smallest principal cosine between the reference's 10 components and the exact leading subspace
                 (for the README; no test asserts it).
"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
GOLD = os.path.join(REPO, "tests", "golden")
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, HERE)
import _pca_fit_ref as fref  # noqa: E402
from gen_golden_pca import load_reference, quiet, write_dataset  # noqa: E402


N_FULL = 24             # genes (and components) of the full regime
MIN_GAP = 2e-3          # its neighbouring eigenvalues are at least this far apart, relative to the largest


def synth(rng, n_cells, n_genes, rank, empty):
    """counts with a planted low-rank structure: Poisson rates exp(factors . loadings) around 0.6 per entry"""
    F = rng.normal(size=(n_cells, rank)) * np.array([1.0, 0.85, 0.7, 0.6, 0.5, 0.4][:rank])
    L = rng.normal(size=(rank, n_genes)) * 0.7
    X = rng.poisson(0.6 * np.exp(F @ L - 0.5)).astype(np.float32)
    for j in empty:
        X[:, j] = 0
    return X


def main(seed=20241017):
    ds_mod = load_reference()
    rng = np.random.default_rng(seed)
    td = tempfile.mkdtemp()
    cells = ["c%d" % i for i in range(300)]
    genes = ["G%d" % i for i in range(120)]
    keep_cells = [i for i in range(300) if i % 11 != 3]
    keep_genes = [i for i in range(120) if i % 9 != 4]
    X = synth(rng, 300, 120, 6, empty=(7,))                      # G7 is kept and has no nonzero value: not a valid gene
    sf = (0.5 + rng.random(300) * 1.5).astype(np.float32)
    fn = os.path.join(td, "sample.h5")
    write_dataset(fn, cells, genes, X, sf, keep_cells, keep_genes)
    out = {"cells": np.array(cells), "genes": np.array(genes), "sf": sf, "keep_cells": np.array(keep_cells, dtype=np.int64),
           "keep_genes": np.array(keep_genes, dtype=np.int64)}
    ci, gi = np.nonzero(X)
    out["cell_ptr"] = np.concatenate([[0], np.cumsum(np.bincount(ci, minlength=300))]).astype(np.int64)
    out["gene"], out["cval"] = gi.astype(np.int32), X[ci, gi].astype(np.float32)
    ds = quiet(ds_mod.Dataset, fn)
    quiet(ds.set_gene_stats)
    valid = [g for g, v in zip(genes, ds.geneStats.valid_gene.values) if v]
    assert "G7" not in valid and "G4" not in valid and len(valid) > 100
    # the full regime's genes: the first random draw of N_FULL valid genes whose covariance has well separated eigenvalues
    # (the projected cells of two exact fits differ by rounding / gap, and a test compares them with the reference's)
    sp_all = quiet(ds.get_scaling_params, valid)
    Yall = np.array([a for _, a in quiet(lambda: list(ds.get_scaled_values(sp_all, disable_tqdm=True)))])
    for draw in range(1000):
        pick = [int(i) for i in rng.permutation(len(valid))]
        lam = np.linalg.eigvalsh(np.cov(Yall[:, pick[:N_FULL]].T))
        if float((np.diff(lam) / lam[-1]).min()) > MIN_GAP:
            break
    else:
        raise SystemExit("no draw of genes with a relative eigenvalue gap above %g: reseed" % MIN_GAP)
    pick = [valid[i] for i in pick]
    asked = {"full": pick[:N_FULL], "trunc": pick[N_FULL:N_FULL + 40] + ["G7", "nobody"]}
    n_comps = {"full": N_FULL, "trunc": 10}
    exact = {}
    for regime in ("full", "trunc"):
        quiet(ds.fit_ipca, asked[regime], n_comps[regime], None, True)
        sp = quiet(ds.get_scaling_params, asked[regime])
        sel = list(sp.index)
        assert sel == ds.ipca.genes and sel == [g for g in asked[regime] if g in set(valid)]
        assert ds.ipca.components_.shape == (n_comps[regime], len(sel)) and ds.ipca.n_samples_seen_ == len(keep_cells)
        Yref = np.array([a for _, a in quiet(lambda: list(ds.get_scaled_values(sp, disable_tqdm=True)))])
        assert Yref.dtype == np.float64
        out[regime + "_asked"], out[regime + "_genes"] = np.array(asked[regime]), np.array(sel)
        out[regime + "_mu"], out[regime + "_sigma"] = sp["mu"].values.astype(np.float64), sp["sigma"].values.astype(np.float64)
        out[regime + "_mean"], out[regime + "_components"] = ds.ipca.mean_.astype(np.float64), ds.ipca.components_.astype(np.float64)
        out[regime + "_explained_variance"] = ds.ipca.explained_variance_.astype(np.float64)
        out[regime + "_Z"] = ds.ipca.transform(Yref).astype(np.float64)
        # the restatement on the stored arrays
        kw, sel2 = fref.fit_call(out, regime)
        assert sel2 == sel
        Y = fref.scaled_rows(**kw)
        assert np.array_equal(Y, Yref)
        mean, cov = fref.mean_cov(Y)
        exact[regime] = (Y, fref.fit(mean, cov, Y.shape[0], cov.shape[0]))
    # ---- full: the reference is exact
    Y, f = exact["full"]
    devs = fref.full_devs(out, f["mean_"], f["explained_variance_"], (Y - f["mean_"]) @ f["components_"].T)
    lam = f["explained_variance_"]
    gap = float(((lam[:-1] - lam[1:]) / lam[0]).min())
    print("full: deviations mean %.3g, explained variance %.3g, projected cells %.3g; smallest relative eigenvalue gap %.3g" % (devs + (gap,)))
    assert 0 < max(devs) < 1e-9, devs
    assert gap > 1e-6 and gap > 0.9 * MIN_GAP, gap
    # ---- trunc: the distance between the reference's subspace and the exact one
    Y, f = exact["trunc"]
    cos = fref.min_cosine(out["trunc_components"], f["components_"][:10])
    print("trunc: smallest principal cosine of the reference's 10 components against the exact ones %.4f" % cos)
    out["fit_full_dev"], out["fit_trunc_cos"], out["full_gap"] = np.float64(max(devs)), np.float64(cos), np.float64(gap)
    fn = os.path.join(GOLD, "pca_fit.npz")
    np.savez_compressed(fn, **out)
    print("wrote %s (%d bytes)" % (fn, os.path.getsize(fn)))


if __name__ == "__main__":
    sys.exit(main())
