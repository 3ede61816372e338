/*
 * nabo_ingest.h -- C ABI of the Matrix Market reader in libnabo_knn.so (MI355X, gfx950).
 *
 * Replaces the per-line Python loop and the per-batch transpose of the reference's mtx_to_h5 (nabo/_io.py:61-235): the
 * text of a `matrix.mtx` is parsed on the device, and the counts come back twice -- as compressed sparse rows of cells
 * (what nabo_cell_qc, nabo_pca_project and nabo_pca_cov read) and as compressed sparse columns of genes (what
 * nabo_gene_stats and nabo_de_test read).  Everything is integer work and does not depend on how the hardware orders
 * anything: the same bytes give the same arrays on every run, however they were fed.
 * Same conventions as nabo_knn.h: 0 or a negative NABO_E_* status, the message in nabo_last_error(), no CPU fallback
 * (NABO_E_NODEVICE without a device).  Every pointer is a host pointer, and every argument is checked on the host
 * before any device call.
 *
 * THE GRAMMAR
 *
 * Header (parsed on the host from the first bytes fed; no length limit).  The first line must start with
 * `%%MatrixMarket`; its words after that, compared without regard to case, must be `matrix coordinate <field> general`
 * with <field> `integer` or `real`.  Anything else is NABO_E_INVALID.  Following lines whose first byte is `%` are
 * comments.  The first other line is the size line, three unsigned integers `n_genes n_cells nnz` separated by blanks.
 * n_genes or n_cells at or above 2^31, or nnz at or above 2^32 - 1, is NABO_E_UNSUPPORTED.
 *
 * Body.  A line is a maximal run of bytes without `\n`; the last line may lack its `\n`.  A blank is a space or a tab;
 * a `\r` directly in front of the `\n`, or at the end of the stream, counts as a blank.  A line of blanks only, or one
 * whose first non-blank byte is `%`, is skipped.  Every other line must be
 *     blanks* digits+ blanks+ digits+ blanks+ digits+ blanks*
 * -- gene, cell, value.  Leading zeros are allowed; signs, decimal points and exponents are not (a `real` file is
 * accepted as long as its values are written as unsigned integers; the message for `3.0` says that real values are not
 * supported).  gene must lie in [1, n_genes], cell in [1, n_cells], value in [0, 2^32 - 1].  A field with more than 19
 * digits after its leading zeros is out of range outright; shorter fields are evaluated in uint64.  A stored zero is
 * kept as an entry, as the reference keeps it.  A body line of more than max_line bytes (its `\n` not counted) is an
 * error, skipped lines included.
 *
 * Errors.  Every grammar or range error is NABO_E_INVALID and its message begins `line N:`, N counted from 1 over the
 * whole file, header lines included; N is the LOWEST bad line.  Within one line the length is judged first, then the
 * first offending byte from the left, then the number of fields, then the ranges of gene, cell and value in this order.
 * More entry lines than nnz is an error of the first line in excess, reported by the feed that uploads it; fewer is an
 * error at finish, with N the last line of the file.  The same (gene, cell) listed twice is an error at finish, and the
 * message names the lowest such pair (by cell, then gene) 1-based: the CSR rule of this library is strictly increasing
 * genes inside a cell.
 * After an error the handle accepts nothing but nabo_mtx_free.
 *
 * Result.  CSR ordered by (cell, gene) ascending, CSC by (gene, cell) ascending, indices 0-based.  The result does not
 * depend on the order of the lines in the file, on how the bytes were fed, on chunk_bytes or on the run.
 *
 * HOW IT RUNS
 *
 * feed buffers bytes in pinned host memory; once chunk_bytes are there, the bytes up to the last `\n` are uploaded and
 * parsed, and the unfinished last line is carried to the front of the buffer.  On the device a line belongs to the tile
 * (tile_bytes of text) in which its first byte lies, and one workgroup owns one tile: the grid of the parse kernel is one
 * workgroup per tile, no workgroup loops over tiles.  The workgroup loads its tile and max_line bytes of look-ahead into
 * LDS with 16-byte loads, builds the `\n` bit masks, and one lane parses the lines that start in its 64 bytes.  Entries
 * are stored in file order: a workgroup scan places them inside the tile, a device-wide exclusive scan of the per-tile
 * counts places the tiles.  An error is recorded with a 64-bit atomicMin of (byte offset of the line << 8 | code), an
 * integer minimum, so the lowest bad line wins whatever the hardware does first.
 * finish sorts the keys (cell << 32 | gene) by the bits in use (rocPRIM radix sort), looks for equal neighbours, builds
 * cell_ptr, and gets the CSC by a stable sort of the gene bits alone with the value as payload and a pointer build; that
 * last stage is also nabo_csr_transpose.
 *
 * Device memory.  With nnz from the size line, C = the chunk size in use and t = ceil((C + max_line + 1) / tile_bytes)
 * tiles, the handle allocates at most
 *     peak(nnz, C) = 32 nnz + 8 (n_cells + 1) + 8 (n_genes + 1) + (C + max_line + 64) + 12 (tile_bytes / 6 + 2) t + 8 (t + 2) + 64
 * bytes plus rocPRIM's temporary storage (for the double-buffered sorts and the scan of t counts), which is queried
 * and added before anything is allocated.  The sum is checked against mem_budget_bytes as soon as the size line is known;
 * exceeding it is NABO_E_NOMEM.
 */
#ifndef NABO_INGEST_H
#define NABO_INGEST_H

#include <stdint.h>

#include "nabo_knn.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nabo_mtx nabo_mtx;

/* A reader on `device`.  chunk_bytes: the text uploaded and parsed at a time; <= 0 means 64 MiB; values below 64 are
 * raised to 64 and values above 1 GiB lowered to 1 GiB.  mem_budget_bytes <= 0 means three quarters of the device memory
 * that is free at this call. */
int nabo_mtx_create(int32_t device, int64_t chunk_bytes, int64_t mem_budget_bytes, nabo_mtx **out);

/* The next n bytes of the file, in ANY split: mid-line, one byte at a time, or all at once.  n = 0 is allowed. */
int nabo_mtx_feed(nabo_mtx *h, const void *bytes, int64_t n);

/* The end of the stream: parses the tail, checks the entry count, sorts, builds both indexes, checks for duplicates.
 * Any of the outputs may be NULL.  Called once. */
int nabo_mtx_finish(nabo_mtx *h, int64_t *n_genes, int64_t *n_cells, int64_t *nnz);

/* After finish.  cell_ptr int64[n_cells + 1], gene int32[nnz], val uint32[nnz]: cell c lists gene[cell_ptr[c] ..
 * cell_ptr[c + 1]), strictly increasing.  An output may be NULL to leave it out. */
int nabo_mtx_get_csr(nabo_mtx *h, int64_t *cell_ptr, int32_t *gene, uint32_t *val);

/* After finish.  gene_ptr int64[n_genes + 1], cell int32[nnz], val uint32[nnz]: gene g lists cell[gene_ptr[g] ..
 * gene_ptr[g + 1]), strictly increasing. */
int nabo_mtx_get_csc(nabo_mtx *h, int64_t *gene_ptr, int32_t *cell, uint32_t *val);

void nabo_mtx_free(nabo_mtx *h);

/* tile_bytes: the bytes of text one workgroup owns; max_line: the longest body line accepted. */
int nabo_mtx_geometry(int32_t *tile_bytes, int32_t *max_line);

/* Device time in ms between HIP events, summed over the chunks: ms[0] upload of the text, ms[1] parse (the parse
 * kernel, the scan of the tile counts and the placement), ms[2] the CSR sort with the duplicate check and cell_ptr,
 * ms[3] the transpose, ms[4] the downloads of get_csr and get_csc so far; the number of chunks parsed. */
int nabo_mtx_last_device_ms(nabo_mtx *h, double ms[5], int64_t *n_chunks);

/* The second half on its own: a CSR of n_rows rows over n_cols columns under the rules of nabo_cell_qc (ptr[0] = 0,
 * monotone; indices in [0, n_cols) and strictly increasing inside a row; float32 values finite and >= 0) to its CSC:
 * out_ptr int64[n_cols + 1], out_idx int32[nnz] (rows ascending inside a column), out_val float32[nnz] (bit copies).
 * n_rows and n_cols below 2^31 - 1, nnz below 2^32 - 1.  Device memory: 24 nnz + 8 (n_rows + 1) + 8 (n_cols + 1) bytes
 * plus rocPRIM's temporary storage. */
int nabo_csr_transpose(int32_t device, int64_t n_rows, int64_t n_cols, const int64_t *ptr, const int32_t *idx,
                       const float *val, int64_t *out_ptr, int32_t *out_idx, float *out_val);

#ifdef __cplusplus
}
#endif

#endif /* NABO_INGEST_H */
