/*
 * nabo_de.h -- C ABI of the Mann-Whitney differential-expression test in libnabo_knn.so (MI355X, gfx950).
 *
 * Replaces the gene x control-group loop of the reference's nabo/_marker.py (run_de_test :12-114, and through it
 * find_cluster_markers :117-169): per gene and per (test set, control set) pair, the expressed fraction, the log2 fold
 * change against the largest values of the control set, the rank-sum statistic U with tie-averaged ranks, the tie term
 * and the two-sided p-value as scipy >= 1.7 `mannwhitneyu(test, ctrl)` gives it (continuity correction, method 'auto').
 * Same conventions as nabo_knn.h: 0 or a negative NABO_E_* status, the message in nabo_last_error(), no CPU fallback
 * (NABO_E_NODEVICE without a device).  Every pointer is a host pointer.
 */
#ifndef NABO_DE_H
#define NABO_DE_H

#include <stdint.h>

#include "nabo_knn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* out_status of a (gene, pair) */
#define NABO_DE_SKIP_GENE 0  /* expressed fraction of the test set below exp_frac_thresh: nothing else was computed */
#define NABO_DE_SKIP_PAIR 1  /* log2_fc below log2_fc_thresh: out_log2_fc is set, no statistic */
#define NABO_DE_ASYMPTOTIC 2 /* tested, p from the normal approximation */
#define NABO_DE_EXACT 3      /* tested, p from the exact distribution of U (n1 <= 8 or n2 <= 8, and no ties) */
#define NABO_DE_EMPTY 4      /* the control set is empty: out_log2_fc is NaN, no statistic (the reference emits a row) */

/* Expression: compressed sparse columns, one column per gene.  Gene g holds cells cell[gene_ptr[g] .. gene_ptr[g+1])
 * (gene_ptr[0] = 0, monotone; inside a column the cells are STRICTLY increasing and in [0, n_cells)) with values
 * val[...]; the value of cell c is (float)(val * sf[c]), one float32 product as in the reference
 * (nabo/_dataset.py:191-193), and 0 for a cell the column does not list.  Every scaled value must be finite and >= 0,
 * NABO_E_INVALID otherwise (a deviation: the reference would rank negative values too; Nabo's normalised counts have
 * none).  The control sets read a second matrix (cell2 / val2 / sf2 over n_cells2 cells, same genes) when gene_ptr2 is
 * not NULL, the first one otherwise.
 *
 * Cell sets: set s is members[set_ptr[s] .. set_ptr[s+1]) (set_ptr[0] = 0, monotone; repeats allowed and counted; a
 * cell may be in several sets).  Pairs: pair p tests set pair_test[p] against control set pair_ctrl[p]; with pair_test
 * NULL there are n_sets - 1 pairs, set 0 against sets 1, 2, ... (n_pairs is then ignored).  A test set must not be
 * empty (NABO_E_INVALID); an empty control set gives NABO_DE_EMPTY.  With a second matrix no set may be test in one
 * pair and control in another.  n1 + n2 < 2^21 per pair (NABO_E_UNSUPPORTED beyond: the tie term is kept in int64).
 *
 * Per gene g and pair p, at [g * n_pairs + p] of every output (all must be given):
 *   nonzero_test = nonzero values of the test set, n1 = its size; exp_frac = nonzero_test / n1 in float64; the gene is
 *                  skipped when exp_frac < exp_frac_thresh;
 *   n2           = min(n1, size of the control set): only the n2 LARGEST control values are used;
 *   log2_fc      = log2(mean test) - log2(mean control), means in float64 over the float32 values (the reference sums
 *                  in float32); +inf when the control mean is 0; the pair is skipped when log2_fc < log2_fc_thresh;
 *   u2           = 2 * U1, U1 the rank-sum statistic of the test sample with tie-averaged ranks (an exact integer);
 *   tie          = sum of t^3 - t over the tie groups of the pooled sample (an exact integer);
 *   z            = (max(U1, U2) - n1 n2 / 2 - 0.5) / sqrt(n1 n2 / 12 * ((n + 1) - tie / (n (n - 1)))), n = n1 + n2,
 *                  float64 operations in this order, none fused;
 *   pval         = min(1, erfc(z / sqrt 2)) with the host's libm, or for NABO_DE_EXACT 2 * P(U >= max(U1, U2)) from the
 *                  distribution of U, clipped to 1 (NABO_E_UNSUPPORTED when C(n1 + n2, n1) >= 2^127);
 *   rbc          = 1 - u2 / (n1 * n2).
 * Entries a status leaves out are 0 (NaN for log2_fc of NABO_DE_EMPTY).
 *
 * Genes are processed in chunks: the per-chunk device buffers (the chunk's nonzeros, 24 bytes per (nonzero, set
 * membership) for the sort, its results) are sized to stay within mem_budget_bytes (<= 0: 2 GiB); a single gene that
 * needs more is NABO_E_NOMEM.  Tables per cell and per membership stay resident beside it; nothing of size
 * cells x genes is allocated. */
int nabo_de_test(int32_t device, int64_t n_genes, int64_t n_cells, const int64_t *gene_ptr, const int32_t *cell,
                 const float *val, const float *sf, int64_t n_cells2, const int64_t *gene_ptr2, const int32_t *cell2,
                 const float *val2, const float *sf2, int64_t n_sets, const int64_t *set_ptr, const int64_t *members,
                 int64_t n_pairs, const int32_t *pair_test, const int32_t *pair_ctrl, double exp_frac_thresh,
                 double log2_fc_thresh, int64_t mem_budget_bytes, int32_t *out_status, int64_t *out_nonzero_test,
                 int64_t *out_n1, int64_t *out_n2, int64_t *out_u2, int64_t *out_tie, double *out_log2_fc, double *out_z,
                 double *out_pval, double *out_rbc);

/* The benchmark's timer (tools/bench_de.py).  Device time in ms, between HIP events and summed over the chunks, of the
 * calling thread's last nabo_de_test -- ms[0] expand (counting, scan and emission of the keys), ms[1] the sort and the
 * segment pointers, ms[2] the rank kernel; uploads and downloads left out -- and the number of gene chunks it took. */
int nabo_de_last_device_ms(double ms[3], int64_t *n_chunks);

#ifdef __cplusplus
}
#endif

#endif /* NABO_DE_H */
