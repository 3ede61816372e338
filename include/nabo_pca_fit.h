/*
 * nabo_pca_fit.h -- C ABI of the exact PCA fit's device half in libnabo_knn.so (MI355X, gfx950): the mean and the sample
 * covariance of the scaled cells.  Included by nabo_pca.h; it is a file of its own so that each header's list of entry
 * points stays pinned by its own test.
 *
 * Replaces the per-cell loop of Dataset.fit_ipca (nabo/_dataset.py:917-983), which densifies every kept cell in Python
 * and feeds sklearn's IncrementalPCA in batches.  The eigen-decomposition of the G x G covariance is host work
 * (nabo_amd/_pca.py, fit_pca_csr).  Conventions as in nabo_pca.h: 0 or a negative NABO_E_* status, the message in
 * nabo_last_error(), no CPU fallback (NABO_E_NODEVICE without a device), host pointers, every argument checked on the
 * host before any device call.
 */
#ifndef NABO_PCA_FIT_H
#define NABO_PCA_FIT_H

#include <stdint.h>

#include "nabo_knn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Mean and sample covariance of the scaled values of the listed cells.
 *
 * The expression matrix (cell_ptr, gene, val, sf), gene_pos, mu, sigma and rows follow exactly the rules of
 * nabo_pca_project (nabo_pca.h): compressed sparse rows with genes strictly increasing inside a cell, every float32
 * product val * sf[cell] finite and >= 0, no position twice in gene_pos, sigma finite and > 0, mu finite, rows may repeat
 * and NULL means all n_cells cells.  A selected gene no raw gene maps to is a `fill_missing` gene: 0 in every cell.
 * New here: n_rows >= 2, NABO_E_INVALID otherwise.  out_mean[G], out_cov[G * G] (row-major), float64.
 *
 * The definition, in float64, with n = n_rows:
 *   y[r][p]   = ((double)(float)(val * sf[cell]) - mu[p]) / sigma[p]   for a listed entry with p = gene_pos[gene] >= 0,
 *   y[r][p]   = (0.0 - mu[p]) / sigma[p]                               for every other p   (the reference's roundings, :912);
 *   mean[p]   = (sum over r of y[r][p]) / n;
 *   cov[p][q] = (sum over r of (y[r][p] - mean[p]) * (y[r][q] - mean[q])) / (n - 1).
 * Two passes: the mean first, then the centred values; never sum(y y^T) - n mean mean^T, which cancels when mu comes
 * from another dataset.
 *
 * The order of the sums is the device's choice, with three guarantees:
 *   - the same call twice gives the same bits (no floating-point atomics anywhere);
 *   - cov[p][q] and cov[q][p] are the same bits (the tiles on and below the diagonal are computed, and mirrored);
 *   - nothing of size n_cells x n_raw_genes is ever allocated.
 *
 * Memory: with Gp = G rounded up to a multiple of 128 and t = (Gp / 128) (Gp / 128 + 1) / 2 tiles, what stays resident
 * is  t * 131072 * (1 + s) + Gp * 2048  bytes, s = min(16, max(1, ceil(1024 / t)))  (the accumulator, the partial tiles
 * of the split cell range, the partial column sums); the rows are processed in chunks whose buffers -- 12 + 8 Gp bytes
 * per row and 8 per listed entry -- fit in what is left of mem_budget_bytes (<= 0: 2 GiB).  If not even one row fits,
 * NABO_E_NOMEM with "budget" in the message. */
int nabo_pca_cov(int32_t device, int64_t n_cells, int64_t n_raw_genes, const int64_t *cell_ptr, const int32_t *gene,
                 const float *val, const float *sf, const int32_t *gene_pos, int64_t n_sel_genes, const double *mu,
                 const double *sigma, int64_t n_rows, const int64_t *rows, int64_t mem_budget_bytes,
                 double *out_mean /* [G] */, double *out_cov /* [G * G] */);

/* The benchmark's timer (tools/bench_pca_fit.py): device ms of the calling thread's last nabo_pca_cov by phase, summed
 * over the chunks -- ms[0] the column sums (with the rows densified for them), ms[1] densifying the centred rows, ms[2]
 * the product (with the sum of its partial tiles and the final division).  nabo_pca_last_device_ms (nabo_pca.h) reports
 * the same call as uploads / all kernels / downloads, and the number of chunks. */
int nabo_pca_cov_last_phase_ms(double ms[3]);

#ifdef __cplusplus
}
#endif

#endif /* NABO_PCA_FIT_H */
