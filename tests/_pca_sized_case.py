"""The sized case of test_pca_gpu.py, in a process of its own so that it runs under a time limit of its own: 300 000
cells x 8 000 raw genes at about 4 % density, 1 500 selected genes, 50 components.  All rows bit-equal between one chunk
and forced chunks, 4 096 seeded rows bit-equal to the restatement, the statistics of all 8 000 genes within the bounds of
test_pca_gpu.py.  Prints the device ms; asserts no speed (no number exists to hold it to)."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import _pca_ref as pref  # noqa: E402

from nabo_amd import _de, _pca  # noqa: E402

EPS = 2.0 ** -53


def make(n_cells, n_raw, per_cell, n_sel, n_comps, seed):
    """per cell, one candidate gene in each of `per_cell` equal strides of the raw genes (strictly increasing), 10 % of
    them dropped again: about per_cell * 0.9 / n_raw density with rows of different lengths"""
    rng = np.random.default_rng(seed)
    stride = n_raw // per_cell
    gene = (np.arange(per_cell, dtype=np.int32) * stride)[None, :] + rng.integers(0, stride, (n_cells, per_cell), dtype=np.int32)
    keep = rng.random((n_cells, per_cell)) < 0.9
    keep[::1000] = False                                         # some cells without any entry
    cell_ptr = np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.int64)
    gene = gene[keep]
    val = (rng.poisson(1.5, gene.shape[0]) + 1).astype(np.float32)
    sf = (0.5 + rng.random(n_cells)).astype(np.float32)
    sel = np.sort(rng.permutation(n_raw)[:n_sel - 10])          # 10 selected genes are in no raw gene: fill_missing genes
    gene_pos = np.full(n_raw, -1, dtype=np.int32)
    gene_pos[sel] = rng.permutation(n_sel)[:n_sel - 10]
    mu, sigma, mean = rng.random(n_sel), 0.5 + rng.random(n_sel), rng.normal(size=n_sel) * 0.1
    comps = rng.normal(size=(n_comps, n_sel)) / np.sqrt(n_sel)
    return (cell_ptr, gene, val, sf), (gene_pos, mu, sigma, mean, comps)


def to_csc(m, n_raw):
    cell_ptr, gene, val, sf = m
    cell = np.repeat(np.arange(sf.shape[0], dtype=np.int32), np.diff(cell_ptr))
    order = np.argsort(gene, kind="stable")                      # stable: the cells of a gene stay increasing
    gene_ptr = np.concatenate([[0], np.cumsum(np.bincount(gene, minlength=n_raw))]).astype(np.int64)
    return gene_ptr, cell[order], val[order], sf


def main():
    n_cells, n_raw, n_sel, n_comps = 300000, 8000, 1500, 50
    m, t = make(n_cells, n_raw, 355, n_sel, n_comps, seed=99)
    out = {"nnz": int(m[1].shape[0]), "density": m[1].shape[0] / (n_cells * n_raw)}
    mm, tt = _pca._csr(m), _pca._tables(*t)
    Z1 = _pca._device_project(mm, *tt, None, mem_budget=8 << 30)
    out["ms_one"], out["chunks_one"] = _pca.last_device_ms()
    Zc = _pca._device_project(mm, *tt, None, mem_budget=96 << 20)
    out["ms_chunked"], out["chunks_chunked"] = _pca.last_device_ms()
    out["chunks_equal"] = bool(np.array_equal(Z1.view(np.int64), Zc.view(np.int64)))
    rows = np.random.default_rng(7).integers(0, n_cells, 4096)
    rows[:3] = [0, 1000, n_cells - 1]                            # an empty cell and the last one among them
    want = pref.project(*m, *t, rows=rows)
    out["rows_equal"] = bool(np.array_equal(Z1[rows].view(np.int64), want.view(np.int64)))
    Zr = _pca._device_project(mm, *tt, np.ascontiguousarray(rows, dtype=np.int64))
    out["rows_call_equal"] = bool(np.array_equal(Zr.view(np.int64), want.view(np.int64)))
    del Z1, Zc
    # ---- the statistics of every gene, over a keep list that drops a tenth of the cells
    csc = to_csc(m, n_raw)
    keep_cells = np.nonzero(np.arange(n_cells) % 10 != 3)[0].astype(np.int64)
    got = _pca._device_stats(_de._csc(csc, "sized"), keep_cells, None)
    out["ms_stats"], out["chunks_stats"] = _pca.last_device_ms()
    ref = pref.gene_stats(*csc, keep_cells=keep_cells)
    n = keep_cells.shape[0]
    out["stats_exact"] = bool(np.array_equal(got["ncells"], ref["ncells"]) and np.array_equal(got["valid"], ref["valid"]))
    out["valid_genes"] = int(ref["valid"].sum())
    for k, bound in (("m", n * EPS), ("nzm", n * EPS), ("variance", 4 * n * EPS)):
        rel = np.abs(got[k] - ref[k]) / np.where(ref[k] != 0, np.abs(ref[k]), 1.0)
        out[k + "_rel"], out[k + "_bound"] = float(rel.max()), bound
    print("RESULT " + json.dumps(out))


if __name__ == "__main__":
    main()
