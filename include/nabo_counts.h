/*
 * nabo_counts.h -- C ABI of the Matrix Market writer and of the remap of count matrices in libnabo_knn.so (MI355X, gfx950).
 *
 * The way out for raw counts and the one primitive behind subsetting and merging them: what the reference does in
 * h5_to_mtx (nabo/_io.py:645-674, one formatted text line per entry in a Python loop), extract_cells_from_h5 (:597-642)
 * and merge_h5 (:502-594, every index through a Python dict).  The writer is the mirror of the reader of nabo_ingest.h:
 * integers to text; the remap renumbers and regroups the entries of a sparse matrix and rebuilds both indexes.  Everything
 * is integer work and does not depend on how the hardware orders anything: the same arguments give the same bytes and the
 * same arrays on every run.
 * Same conventions as nabo_knn.h: 0 or a negative NABO_E_* status, the message in nabo_last_error(), no CPU fallback
 * (NABO_E_NODEVICE without a device).  Every pointer is a host pointer, and every argument is checked on the host before
 * any device call.  A compressed sparse argument follows the library's rule: ptr[0] = 0, ptr monotone, indices in range
 * and strictly increasing inside a list.  Values are 32-bit payloads here: the writer reads them as uint32, the remap
 * copies them bit for bit (a float32 comes back with its bits).
 *
 * THE TEXT (nabo_mtxw_*)
 *
 * Banner `%%MatrixMarket matrix coordinate integer general\n`; then `comments` as given; then the size line
 * "%d %d %d\n" of n_genes, n_cells, nnz; then for cell c = 0, 1, ... and its genes in ascending order one line per entry,
 * "%d %d %d\n" of gene + 1, c + 1, value.  Numbers are plain decimal, no leading zeros, no sign, one space between them.  A
 * stored zero is written.  With blank_line_for_empty_cell a cell without entries contributes a single `\n` (what the
 * reference's '\n'.join([]) + '\n' does; the reader of nabo_ingest.h skips such a line), without it nothing.
 * Limits: n_genes and n_cells below 2^31, nnz below 2^32 - 1 (as for the reader), and at most 130150524 entries in one
 * cell (its text is addressed with 32 bits inside the cell): NABO_E_UNSUPPORTED beyond.
 * total_bytes is exact and known after create.  The bytes delivered do not depend on cap, on chunk_bytes, on the device
 * or on the run, and nabo_mtx_* given them returns the matrix that was written.
 *
 * HOW IT RUNS
 *
 * create uploads the matrix, and a length pass gives every entry the byte offset of its line inside its cell (32 bits)
 * and every cell its number of bytes: 16 lanes walk one cell, a cell of more than long_cell entries gets a workgroup.
 * An exclusive scan (rocPRIM) turns the cells' bytes into 64-bit offsets; the last one is the size of the body.
 * read formats the body chunk_bytes at a time.  One workgroup owns one tile (tile_bytes of text): it finds the line that
 * holds the tile's first byte by binary search over the cell offsets and then over the entry offsets of that cell,
 * formats every line that has a byte in the tile into LDS, and stores exactly its tile with 16-byte stores.  A line that
 * straddles the end of a tile (or of a chunk) is therefore formatted by both neighbours, and each stores its own part:
 * no two workgroups ever write the same byte, nothing is carried from tile to tile or chunk to chunk, and there is no
 * atomic anywhere.  The chunk is copied to pinned host memory and handed out in reads of any cap.
 *
 * Device memory.  With C the chunk size in use, L the number of cells of more than long_cell entries:
 *     peak(nnz, n_cells, C) = 12 nnz + 24 (n_cells + 1) + 4 L + (C + 16) + 64
 * bytes plus rocPRIM's temporary storage for the scan, which is queried and added before anything is allocated.  The sum is
 * checked against mem_budget_bytes first; exceeding it is NABO_E_NOMEM.
 *
 * THE REMAP (nabo_counts_remap)
 *
 * Output row r is input row row_src[r] (repeats allowed) with every index j replaced by col_map[j], entries whose
 * col_map is -1 dropped.  The caller sizes out_idx, out_val, csc_idx and csc_val by the bound B = the sum over r of the
 * length of row row_src[r]; B must be below 2^32 - 1 (NABO_E_UNSUPPORTED), n_rows, n_cols, n_out_rows and n_out_cols below
 * 2^31 - 1.  The true number of entries comes back in out_nnz.
 * Output: out_ptr int64[n_out_rows + 1], out_idx strictly increasing inside a row; csc_ptr int64[n_out_cols + 1], csc_idx
 * (the rows) strictly increasing inside a column.  Two kept columns of one input row that map to the same output column
 * are NABO_E_INVALID; the message names the lowest such (output row, output column), 0-based, found by an integer
 * atomicMin as the reader finds its duplicate, so the verdict does not depend on the run.
 * On the device: 16 lanes count the kept entries of an output row, a scan places the rows, the same lanes write the keys
 * (output row << 32 | new column) with the value as payload; the keys are sorted over the bits in use -- not at all when
 * col_map does not decrease over the columns it keeps, which the host sees --, equal neighbours are the duplicates, and the
 * transpose stage of the reader gives the CSC.
 * Device memory: 8 nnz + 8 (n_rows + 1) + 4 n_cols + 24 (n_out_rows + 1) + 28 B + 8 (n_out_cols + 1) + 64 bytes plus rocPRIM's
 * temporary storage.
 */
#ifndef NABO_COUNTS_H
#define NABO_COUNTS_H

#include <stdint.h>

#include "nabo_knn.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nabo_mtxw nabo_mtxw;

/* A writer of the matrix (cell_ptr int64[n_cells + 1], gene int32[nnz], val uint32[nnz]) on `device`.  comments: NULL, or
 * whole lines each starting with '%' and ending in '\n'.  chunk_bytes: the text that exists on the device at a time; <= 0
 * means 64 MiB; values below 64 are raised to 64, values above 1 GiB lowered to 1 GiB, and the value is rounded up to a
 * whole number of 16 bytes.  mem_budget_bytes <= 0 means three quarters of the device memory that is free at this call.
 * The arrays are not read after create returns.  total_bytes may be NULL. */
int nabo_mtxw_create(int32_t device, int64_t n_genes, int64_t n_cells, const int64_t *cell_ptr, const int32_t *gene, const uint32_t *val,
                     const char *comments, int32_t blank_line_for_empty_cell, int64_t chunk_bytes, int64_t mem_budget_bytes, nabo_mtxw **out,
                     int64_t *total_bytes);

/* The next bytes of the text: at most cap of them, ANY cap >= 1; *n is how many were written to buf: cap until the text
 * runs out, 0 at the end.  A read formats as many chunks as it needs. */
int nabo_mtxw_read(nabo_mtxw *h, void *buf, int64_t cap, int64_t *n);

/* Device time in ms between HIP events: ms[0] the upload of the matrix, ms[1] the length pass and the scan, ms[2] the
 * format kernel and ms[3] the download of the text, both summed over the chunks formatted so far; their number. */
int nabo_mtxw_last_device_ms(nabo_mtxw *h, double ms[4], int64_t *n_chunks);

void nabo_mtxw_free(nabo_mtxw *h);

/* tile_bytes: the text one workgroup of the format kernel owns; min_chunk: the smallest chunk_bytes in use; long_cell: a
 * cell of more entries gets a workgroup of its own in the length pass; max_line: the longest line there is. */
int nabo_mtxw_geometry(int32_t *tile_bytes, int32_t *min_chunk, int32_t *long_cell, int32_t *max_line);

/* The remap (see above).  csc_ptr, csc_idx and csc_val: all three NULL to leave the CSC out. */
int nabo_counts_remap(int32_t device, int64_t n_rows, int64_t n_cols, const int64_t *ptr, const int32_t *idx, const uint32_t *val,
                      int64_t n_out_rows, const int64_t *row_src, int64_t n_out_cols, const int32_t *col_map, int64_t *out_nnz,
                      int64_t *out_ptr, int32_t *out_idx, uint32_t *out_val, int64_t *csc_ptr, int32_t *csc_idx, uint32_t *csc_val);

#ifdef __cplusplus
}
#endif

#endif /* NABO_COUNTS_H */
