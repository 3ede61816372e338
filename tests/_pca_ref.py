"""Plain restatements of include/nabo_pca.h for the tests and for tools/gen_golden_pca.py: the projection as the
header's literal sequential loop (vectorised across rows' components, never across a row's entries), the gene
statistics with math.fsum.  numpy's float64 `+`, `-`, `*`, `/` are single IEEE operations, nothing is fused."""
import json
import math

import numpy as np


def bias_of(mu, sigma, mean, components):
    """bias[c] = sum over p ascending, from 0.0, of ((0.0 - mu[p]) / sigma[p] - mean[p]) * components[c][p]"""
    mu, sigma, mean = (np.asarray(x, dtype=np.float64) for x in (mu, sigma, mean))
    comp = np.asarray(components, dtype=np.float64)
    acc = np.zeros(comp.shape[0], dtype=np.float64)
    for p in range(mu.shape[0]):
        a = (0.0 - mu[p]) / sigma[p]
        b = a - mean[p]
        acc = acc + b * comp[:, p]
    return acc


def project(cell_ptr, gene, val, sf, gene_pos, mu, sigma, mean, components, rows=None):
    """Z[len(rows), C]: per row, bias, then one addition per listed entry of a selected gene, in stored order"""
    cell_ptr, gene = np.asarray(cell_ptr, dtype=np.int64), np.asarray(gene, dtype=np.int64)
    val, sf = np.asarray(val, dtype=np.float32), np.asarray(sf, dtype=np.float32)
    gene_pos, sigma = np.asarray(gene_pos, dtype=np.int64), np.asarray(sigma, dtype=np.float64)
    comp = np.ascontiguousarray(np.asarray(components, dtype=np.float64).T)       # [G, C]
    bias = bias_of(mu, sigma, mean, components)
    rows = np.arange(cell_ptr.shape[0] - 1) if rows is None else np.asarray(rows, dtype=np.int64)
    Z = np.empty((rows.shape[0], comp.shape[1]), dtype=np.float64)
    for r, c in enumerate(rows.tolist()):
        acc = bias.copy()
        for e in range(int(cell_ptr[c]), int(cell_ptr[c + 1])):
            p = int(gene_pos[gene[e]])
            if p < 0:
                continue
            x = np.float32(val[e] * sf[c])                      # one float32 product
            s = np.float64(x) / sigma[p]
            acc = acc + s * comp[p]
        Z[r] = acc
    return Z


def gene_stats(gene_ptr, cell, val, sf, keep_cells=None, keep_genes=None):
    """the header's statistics with exactly rounded sums (math.fsum)"""
    gene_ptr, cell = np.asarray(gene_ptr, dtype=np.int64), np.asarray(cell, dtype=np.int64)
    val, sf = np.asarray(val, dtype=np.float32), np.asarray(sf, dtype=np.float32)
    n_genes, n_cells = gene_ptr.shape[0] - 1, sf.shape[0]
    kept = np.ones(n_cells, dtype=bool)
    if keep_cells is not None:
        kept[:] = False
        kept[np.asarray(keep_cells, dtype=np.int64)] = True
    n = int(kept.sum())
    out = {"ncells": np.zeros(n_genes, np.int64), "valid": np.zeros(n_genes, np.uint8), "m": np.zeros(n_genes), "nzm": np.zeros(n_genes),
           "variance": np.zeros(n_genes)}
    for g in range(n_genes):
        if keep_genes is not None and not keep_genes[g]:
            continue
        c = cell[gene_ptr[g]:gene_ptr[g + 1]]
        x = (val[gene_ptr[g]:gene_ptr[g + 1]] * sf[c])[kept[c]]
        assert x.dtype == np.float32                            # one float32 product per entry
        ncells = int((x > 0).sum())
        if ncells == 0:
            continue
        x = x.astype(np.float64)
        s = math.fsum(x.tolist())
        m = s / n
        out["ncells"][g], out["valid"][g], out["m"][g], out["nzm"][g] = ncells, 1, m, s / ncells
        dev = x - m                                              # float64, one rounding each, as the device's two operations
        out["variance"][g] = (math.fsum((dev * dev).tolist()) + (n - x.shape[0]) * (m * m)) / n
    return out


# ---- the golden file (tests/golden/pca.npz, tools/gen_golden_pca.py) --------------------------------------------------
def csr_of(d, prefix):
    return d[prefix + "_cell_ptr"], d[prefix + "_gene"], d[prefix + "_cval"], d[prefix + "_sf"]


def csc_of(d, prefix):
    return d[prefix + "_gene_ptr"], d[prefix + "_cell"], d[prefix + "_val"], d[prefix + "_sf"]


def keep_mask(d, prefix):
    m = np.zeros(len(d[prefix + "_genes"]), dtype=np.uint8)
    m[d[prefix + "_keep_genes"]] = 1
    return m


def gene_pos_of(raw_genes, selected):
    """position of every raw gene among `selected` or -1 (a name the file holds twice maps through its LAST index, as the
    reference's geneIdx does), and the selected genes the file does not hold"""
    last = {str(g): i for i, g in enumerate(raw_genes)}
    pos = np.full(len(raw_genes), -1, dtype=np.int32)
    missing = []
    for n, g in enumerate(selected):
        if str(g) in last:
            pos[last[str(g)]] = n
        else:
            missing.append(n)
    return pos, missing


def projection_calls(d):
    """every golden projection: (name, dataset prefix, keyword arguments of the projection, the reference's Z)"""
    sel = [str(x) for x in d["pca_genes"]]
    out = []
    for name, prefix in (("ref", "r"), ("target", "t")):
        pos, _ = gene_pos_of(d[prefix + "_genes"], sel)
        cp, gene, val, sf = csr_of(d, prefix)
        kw = dict(cell_ptr=cp, gene=gene, val=val, sf=sf, gene_pos=pos, mu=d["pca_mu"], sigma=d["pca_sigma"], mean=d["pca_mean"],
                  components=d["pca_components"], rows=d[prefix + "_keep_cells"])
        out.append((name, prefix, kw, d[prefix + "_Z"]))
    return out


def row_dev(ref, got):
    """the largest ||reference row - row||inf / max(1, ||reference row||inf)"""
    ref, got = np.asarray(ref), np.asarray(got)
    if not ref.shape[0]:
        return 0.0
    return float((np.abs(ref - got).max(axis=1) / np.maximum(1.0, np.abs(ref).max(axis=1))).max())


def stats_devs(ref, got):
    """largest relative differences of m, nzm, variance over the valid genes"""
    v = np.asarray(ref["valid"]).astype(bool)

    def rel(a, b):
        a, b = np.asarray(a, dtype=np.float64)[v], np.asarray(b, dtype=np.float64)[v]
        return float((np.abs(a - b) / np.where(a != 0, np.abs(a), 1.0)).max()) if a.size else 0.0
    return rel(ref["m"], got["m"]), rel(ref["nzm"], got["nzm"]), rel(ref["variance"], got["variance"])


def golden_stats(d):
    """the reference's geneStats of the reference sample as arrays over the raw genes (0 where a gene is not valid)"""
    return {k: d["r_stats_" + k] for k in ("ncells", "valid", "m", "nzm", "variance")}


def meta(d):
    return json.loads(str(d["meta"]))
