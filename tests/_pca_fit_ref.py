"""Plain restatement of include/nabo_pca_fit.h and of the host logic of nabo_amd._pca._fit_from_csr, for the tests and for
tools/gen_golden_pca_fit.py: the scaled values y, their mean and sample covariance from the definition with exactly
rounded sums (math.fsum), then eigh / order / clipping / sign rule.  numpy's float64 `-`, `*`, `/` are single IEEE
operations, nothing is fused."""
import math

import numpy as np

EPS = 2.0 ** -53


def scaled_rows(cell_ptr, gene, val, sf, gene_pos, mu, sigma, rows=None):
    """y[len(rows), G]: (0.0 - mu) / sigma everywhere, ((double)(float)(val * sf[cell]) - mu) / sigma at the listed selected genes"""
    cell_ptr, gene = np.asarray(cell_ptr, dtype=np.int64), np.asarray(gene, dtype=np.int64)
    val, sf = np.asarray(val, dtype=np.float32), np.asarray(sf, dtype=np.float32)
    gene_pos, mu, sigma = np.asarray(gene_pos, dtype=np.int64), np.asarray(mu, dtype=np.float64), np.asarray(sigma, dtype=np.float64)
    rows = np.arange(cell_ptr.shape[0] - 1) if rows is None else np.asarray(rows, dtype=np.int64)
    base = (0.0 - mu) / sigma
    Y = np.empty((rows.shape[0], mu.shape[0]), dtype=np.float64)
    for r, c in enumerate(rows.tolist()):
        Y[r] = base
        e = slice(int(cell_ptr[c]), int(cell_ptr[c + 1]))
        p = gene_pos[gene[e]]
        x = val[e] * sf[c]
        assert x.dtype == np.float32                            # one float32 product per entry
        Y[r, p[p >= 0]] = (x[p >= 0].astype(np.float64) - mu[p[p >= 0]]) / sigma[p[p >= 0]]
    return Y


def mean_cov(Y):
    """the header's definition with exactly rounded sums: mean = fsum(y) / n; cov = fsum((y - mean_p) * (y - mean_q)) / (n - 1),
    every centred value and every product rounded once"""
    n, G = Y.shape
    mean = np.array([math.fsum(col) for col in Y.T.tolist()], dtype=np.float64) / n
    Yc = Y - mean
    cov = np.empty((G, G), dtype=np.float64)
    for p in range(G):
        prods = (Yc[:, p:p + 1] * Yc[:, :p + 1]).T.tolist()
        for q in range(p + 1):
            cov[p, q] = cov[q, p] = math.fsum(prods[q]) / (n - 1)
    return mean, cov


def exact_mean_cov(Y):
    """mean_cov for the exact-arithmetic cases at sizes where a Python fsum per entry takes too long, in integers: the
    values y of n rows (a power of two) are multiples of 1 / K, K = 4 n, and every column sums to 0, so mean = 0 and
    cov = ((Yi^T Yi) / K^2) / (n - 1) with Yi = K y.  Every partial sum of the product is an integer below 2^53, so the
    float64 matrix product is exact in any order; the division by K^2 is by a power of two, the last one rounds once."""
    n = Y.shape[0]
    K = 4 * n
    assert n & (n - 1) == 0
    Yi = np.rint(Y * K)
    assert np.array_equal(Yi, Y * K) and np.array_equal(Yi / K, Y)
    assert not Yi.sum(axis=0).any()
    assert n * float(np.abs(Yi).max()) ** 2 < 2.0 ** 53
    P = Yi.T @ Yi
    assert np.abs(P).max() < 2.0 ** 53
    return np.zeros(Y.shape[1], dtype=np.float64), (P / float(K * K)) / (n - 1)


def bounds(Y, mean):
    """(e[G], B[G, G]): |mean - exact| <= e_p = n eps A_p with A_p = sum_r |y[r][p]| / n, and
    |cov[p][q] - exact| <= B = (4 n eps s'_p s'_q + n e_p e_q) / (n - 1), s_p = sqrt(sum_r (y[r][p] - mean[p])^2),
    s'_p = s_p + sqrt(n) e_p (the issue's derivation: any order of n terms is within n eps of the exact sum relative to the
    sum of magnitudes, which Cauchy-Schwarz bounds by s_p s_q)"""
    n = Y.shape[0]
    A = np.array([math.fsum(col) for col in np.abs(Y).T.tolist()]) / n
    e = n * EPS * A
    Yc = Y - mean
    s = np.sqrt(np.array([math.fsum(col) for col in (Yc * Yc).T.tolist()]))
    s1 = s + math.sqrt(n) * e
    return e, (4 * n * EPS * np.outer(s1, s1) + n * np.outer(e, e)) / (n - 1)


def fit(mean, cov, n, n_comps):
    """the host logic of _fit_from_csr, restated: eigh, eigenvalues descending (equal ones in eigh's order, reversed), clipped
    at 0 in the reported variances, svd_flip(u_based_decision=False) signs"""
    lam, vec = np.linalg.eigh(np.asarray(cov, dtype=np.float64))
    order = np.arange(lam.shape[0])[::-1][:n_comps]
    comp = np.array([vec[:, j] for j in order])
    for c in range(comp.shape[0]):
        j = int(np.argmax(np.abs(comp[c])))
        if comp[c, j] < 0:
            comp[c] = -comp[c]
    ev = np.where(lam[order] < 0, 0.0, lam[order])
    var = np.diag(cov).copy()
    return {"mean_": np.asarray(mean, dtype=np.float64), "components_": comp, "explained_variance_": ev,
            "explained_variance_ratio_": ev / var.sum(), "singular_values_": np.sqrt(ev * (n - 1)), "var_": var}


def min_cosine(A, B):
    """the smallest principal cosine between the row spaces of A and B (orthonormal rows)"""
    return float(np.linalg.svd(np.asarray(A) @ np.asarray(B).T, compute_uv=False).min())


# ---- the golden file (tests/golden/pca_fit.npz, tools/gen_golden_pca_fit.py) ---------------------------------------
def fit_call(d, regime):
    """keyword arguments of pca_cov_csr for a golden regime ("full" or "trunc"), and its selected genes"""
    sel = [str(x) for x in d[regime + "_genes"]]
    last = {str(g): i for i, g in enumerate(d["genes"])}
    pos = np.full(len(d["genes"]), -1, dtype=np.int32)
    for n, g in enumerate(sel):
        if g in last:
            pos[last[g]] = n
    return dict(cell_ptr=d["cell_ptr"], gene=d["gene"], val=d["cval"], sf=d["sf"], gene_pos=pos, mu=d[regime + "_mu"],
                sigma=d[regime + "_sigma"], rows=d["keep_cells"]), sel


def row_dev(ref, got):
    """the largest ||reference row - row||inf / max(1, ||reference row||inf), as tests/_pca_ref.py"""
    ref, got = np.asarray(ref), np.asarray(got)
    return float((np.abs(ref - got).max(axis=1) / np.maximum(1.0, np.abs(ref).max(axis=1))).max())


def full_devs(d, mean, ev, Z):
    """deviations of a fit from the reference's regime (a): mean_, explained_variance_ relative to the largest, projected
    kept cells by row_dev"""
    return (float(np.abs(mean - d["full_mean"]).max()), float(np.abs(ev - d["full_explained_variance"]).max() / d["full_explained_variance"].max()),
            row_dev(d["full_Z"], Z))
