/*
 * nabo_qc.h -- C ABI of the per-cell quality-control sums in libnabo_knn.so (MI355X, gfx950).
 *
 * Replaces the per-cell Python loops in front of Dataset.filter_data and Dataset.set_sf (nabo/_dataset.py:234-258,
 * :208-232, :369-405, :548-592): the total of a cell, the number of genes it lists, and the cumulative expression of
 * gene classes (mitochondrial, ribosomal, the kept genes) come from ONE pass over the cells.  Thresholds, percentages
 * and size factors are not computed here: they are n_cells-long float32 expressions of the host (nabo_amd/_qc.py).
 * Same conventions as nabo_knn.h: 0 or a negative NABO_E_* status, the message in nabo_last_error(), no CPU fallback
 * (NABO_E_NODEVICE without a device).  Every pointer is a host pointer, and every argument is checked on the host
 * before any device call.
 */
#ifndef NABO_QC_H
#define NABO_QC_H

#include <stdint.h>

#include "nabo_knn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Per-cell sums over the listed entries, all and by gene class.
 *
 * Expression: compressed sparse rows with the layout and the rules of nabo_pca_project (nabo_pca.h), without size
 * factors: cell i lists the raw genes gene[cell_ptr[i] .. cell_ptr[i+1]) (cell_ptr[0] = 0, monotone; inside a cell the
 * genes are STRICTLY increasing and in [0, n_raw_genes)) with values val[...], float32, finite and >= 0.
 * gene_class[n_raw_genes]: bit c (c < n_classes, n_classes in [0, 8]) says that the gene belongs to class c; higher bits
 * are ignored; it may be NULL when n_classes is 0.
 * rows[n_rows]: the cells, in output order; repeats are allowed; NULL means all n_cells cells in order (n_rows is then
 * ignored).  out_n_entries[n_rows], int64; out_sums[n_rows * (1 + n_classes)], float64, row-major.
 *
 * The definition, for row r over cell i with its n listed entries e = 0 .. n-1 in stored order:
 *   out_n_entries[r]   = n;
 *   out_sums[r][0]     = the sum of (double)val over all entries;
 *   out_sums[r][1 + c] = the sum of (double)val over the entries whose gene has bit c set.
 * Every sum is float64 and is taken in this fixed order: 16 partial sums s[0..15] start at 0.0, and entry e is added
 * to s[e mod 16] in ascending e (an entry outside the class adds 0.0); then for d = 8, 4, 2, 1, in this order,
 * s[j] = s[j] + s[j xor d] for every j at once, and the result is s[0].  There are no atomics and the order does not
 * depend on the chunking, so the same input gives the same bits on every run.  (The reference reduces in float32:
 * for integer counts with totals below 2^24 both are exact, hence equal; elsewhere the difference is a deviation,
 * measured in tests/golden/qc.npz, `tot_dev`.)
 *
 * Rows are processed in chunks: the per-chunk device buffers (8 bytes per listed entry, 16 + 8 (1 + n_classes) bytes
 * per row) are sized to stay within mem_budget_bytes (<= 0: 2 GiB); a single row that needs more is NABO_E_NOMEM.  The
 * class table (n_raw_genes bytes) stays resident beside them; a workgroup keeps it in LDS when n_raw_genes <= 65536 and
 * reads it through L2 otherwise. */
int nabo_cell_qc(int32_t device, int64_t n_cells, int64_t n_raw_genes, const int64_t *cell_ptr, const int32_t *gene,
                 const float *val, int32_t n_classes, const uint8_t *gene_class, int64_t n_rows, const int64_t *rows,
                 int64_t mem_budget_bytes, int64_t *out_n_entries, double *out_sums);

/* The benchmark's timer (tools/bench_qc.py).  Device time in ms, between HIP events and summed over the chunks, of the
 * calling thread's last nabo_cell_qc -- ms[0] the uploads, ms[1] the kernel, ms[2] the download -- and the number of
 * chunks that call took. */
int nabo_qc_last_device_ms(double ms[3], int64_t *n_chunks);

#ifdef __cplusplus
}
#endif

#endif /* NABO_QC_H */
