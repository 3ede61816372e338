/*
 * nabo_pca.h -- C ABI of the PCA projection of sparse cells and of the per-gene statistics in libnabo_knn.so (MI355X,
 * gfx950).
 *
 * Replaces the two per-item Python loops in front of every Nabo workflow: the per-cell loop of Dataset.transform_pca
 * (nabo/_dataset.py:985-1033) over get_scaled_values (:846-915), and the per-gene loop of set_gene_stats (:594-637)
 * that get_scaling_params (:814-844) reads.  Same conventions as nabo_knn.h: 0 or a negative NABO_E_* status, the
 * message in nabo_last_error(), no CPU fallback (NABO_E_NODEVICE without a device).  Every pointer is a host pointer,
 * and every argument is checked on the host before any device call.
 */
#ifndef NABO_PCA_H
#define NABO_PCA_H

#include <stdint.h>

#include "nabo_knn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Projects sparse cells onto PCA components: get_scaled_values (nabo/_dataset.py:870-913) followed by
 * transformer.transform([a]) (:1028), without the dense vector in between.
 *
 * Expression: compressed sparse rows, one row per cell.  Cell i lists the raw genes gene[cell_ptr[i] .. cell_ptr[i+1])
 * (cell_ptr[0] = 0, monotone; inside a cell the genes are STRICTLY increasing and in [0, n_raw_genes)) with values
 * val[...], float32, finite and >= 0; sf[n_cells] holds the size factors, and every float32 product val * sf[cell]
 * must be finite and >= 0 (the reference's `a * self.sf[i]`, :912).
 * gene_pos[n_raw_genes]: the position of a raw gene among the G selected genes, or -1; no position may appear twice.
 * A selected gene no raw gene maps to is a `fill_missing` gene (:896-910): it is 0 in every cell.
 * mu[G], sigma[G]: the scaling parameters, float64.  sigma must be finite and > 0, NABO_E_INVALID otherwise (a
 * deviation: the reference would write inf / NaN).  mean[G], components[C * G] (row c holds component c): the
 * transformer's mean_ and components_, float64, in sklearn's layout.
 * rows[n_rows]: the cells to project, in output order (the reference's keepCellsIdx); repeats are allowed; NULL means
 * all n_cells cells in order (n_rows is then ignored).  out_z[n_rows * C], float64.
 *
 * The definition, in float64, one operation at a time, nothing fused:
 *   bias[c] = sum over p = 0 .. G-1, ascending, starting from 0.0, of ((0.0 - mu[p]) / sigma[p] - mean[p]) * components[c][p]
 *   Z[r][c] = bias[c], then for every listed entry of the row with p = gene_pos[gene] >= 0, IN STORED ORDER,
 *             Z[r][c] = Z[r][c] + ((double)(float)(val * sf[cell]) / sigma[p]) * components[c][p]
 * A gene without an entry contributes through bias alone.  (The reference rounds ((x - mu) / sigma - mean) per gene and
 * multiplies through BLAS in another order; the difference is measured in tests/golden/pca.npz, `proj_dev`.)
 * Zeros are never materialised and nothing of size cells x genes is allocated.
 *
 * Rows are processed in chunks: the per-chunk device buffers (8 bytes per listed entry, 12 + 8 C bytes per row) are
 * sized to stay within mem_budget_bytes (<= 0: 2 GiB); a single row that needs more is NABO_E_NOMEM.  The tables per
 * gene (G * C * 8 bytes and smaller ones) stay resident beside them. */
int nabo_pca_project(int32_t device, int64_t n_cells, int64_t n_raw_genes, const int64_t *cell_ptr, const int32_t *gene,
                     const float *val, const float *sf, const int32_t *gene_pos, int64_t n_sel_genes, const double *mu,
                     const double *sigma, const double *mean, int32_t n_comps, const double *components, int64_t n_rows,
                     const int64_t *rows, int64_t mem_budget_bytes, double *out_z);

/* Per-gene statistics of the normalised values: set_gene_stats (nabo/_dataset.py:594-637).
 *
 * Expression: compressed sparse columns with the layout and the rules of nabo_de.h (gene_ptr[n_genes + 1], cell, val,
 * sf[n_cells]; cells strictly increasing inside a column; every float32 product finite and >= 0).
 * keep_cells[n_keep]: the cells that count (the reference's keepCellsIdx), in [0, n_cells), no repeats; NULL means all
 * cells (n_keep is then ignored).  At least one cell must count.  keep_genes[n_genes]: nonzero for a gene to compute
 * (keepGenesIdx); NULL means all genes.
 *
 * With x = (float)(val * sf[cell]) over the kept cells a column lists, `listed` their number and n the number of kept
 * cells, per gene g:
 *   out_ncells[g]   = the number of x > 0;
 *   out_valid[g]    = 1 when the gene is kept and ncells > 0, else 0 (the reference's valid_gene);
 *   out_m[g]        = (sum of x) / n;
 *   out_nzm[g]      = (sum of the x > 0) / ncells;
 *   out_variance[g] = (sum over the listed x of (x - m)^2 + (n - listed) * m^2) / n, the population variance in two passes.
 * The sums are float64 over float32 values, in an order the device chooses (the reference reduces in float32).  Every
 * output of a gene that is not valid is 0.  All outputs must be given. */
int nabo_gene_stats(int32_t device, int64_t n_genes, int64_t n_cells, const int64_t *gene_ptr, const int32_t *cell,
                    const float *val, const float *sf, int64_t n_keep, const int64_t *keep_cells, const uint8_t *keep_genes,
                    int64_t *out_ncells, uint8_t *out_valid, double *out_m, double *out_nzm, double *out_variance);

/* The benchmark's timer (tools/bench_pca.py).  Device time in ms, between HIP events and summed over the chunks, of the
 * calling thread's last nabo_pca_project -- ms[0] the uploads, ms[1] the kernel, ms[2] the download of Z -- or of its
 * last nabo_gene_stats -- ms[1] the kernel, ms[0] = ms[2] = 0 -- or of its last nabo_pca_cov (nabo_pca_fit.h) -- ms[0]
 * the uploads, ms[1] all kernels, ms[2] the downloads -- and the number of chunks that call took. */
int nabo_pca_last_device_ms(double ms[3], int64_t *n_chunks);

#ifdef __cplusplus
}
#endif

/* the exact PCA fit's device half: mean and covariance of the scaled cells */
#include "nabo_pca_fit.h"

#endif /* NABO_PCA_H */
